// Posterior decoding over a phoneme graph (ppg_posterior): the sum over all paths of ppg_viterbi's graph
// where ppg_viterbi takes the best one.  With LSE = log sum exp, LSE of nothing = -inf, and e the prepared frame of
// align_prepare at sym[n]:
//   alpha[0, n] = e[0, n] + initial[n]
//   alpha[t, n] = e[t, n] + LSE(alpha[t-1, n] + stay[n], alpha[t-1, src[j]] + w[j] for every in-arc j)
//   total       = LSE over n of (alpha[T-1, n] + final[n])
//   beta[T-1, n] = final[n]
//   beta[t, n]  = LSE(stay[n] + e[t+1, n] + beta[t+1, n], w + e[t+1, m] + beta[t+1, m] for every out-arc n -> m)
//   gamma[t, n] = exp(alpha[t, n] + beta[t, n] - Z_t), Z_t = LSE over n of (alpha[t, n] + beta[t, n])
//   post[p, t]  = the sum of gamma[t, n] over the states with sym[n] = p
//
// Arithmetic: fp32 in the log domain.  A row is kept less the maxima of the rows before it: the kernels hold
//   a[t, n] = alpha[t, n] - C[t],  C[t] = m[0] + ... + m[t-1] in float64,  m[t] = max over n of a[t, n]
// and frame t+1 takes m[t] off once per state, after its LSE (LSE(x - m) = LSE(x) - m), so a row is written once and no
// value of it is ever larger in magnitude than one frame's step.  b is kept the same way, and since gamma is normalised
// per frame every constant of a row cancels there: only `total` needs C, and leaves as C[T-1] + LSE(a[T-1] + final) in
// float64.  One LSE is the online form: a running maximum `top` and the sum of exp(c - top), one v_exp_f32 per
// candidate.  -inf + finite = -inf; a candidate of -inf adds 0 without a subtraction of two infinities, and a state
// nothing reaches stays -inf: no NaN arises from weights that are finite or -inf.
//
// Kernels, beside align_prepare and viterbi_check, which ppg_align.hip launches for this unit:
//   posterior_check     one wave per GRAPH: the out-arc lists get the tests viterbi_check makes of the in-arc lists
//                       (no limit on the out-degree), and must hold as many arcs as the in-arc lists.
//   posterior_forward   one wave per utterance, time the serial loop, as viterbi_programme: the row of frame t-1 in two
//                       LDS buffers, what a state keeps in LDS beside it, the in-arcs in LDS up to PHELD of them, the
//                       prepared frames staged 32 at a time.  G = 1 takes the graphs of at most 64 states (lane n has
//                       state n), G = 4 the larger ones (256 states a pass, 16-byte LDS operations); a launch of either
//                       leaves the other's items alone, so what an item computes never depends on its neighbours.
//                       Per frame: the LSE per state, the row to the workspace, the wave-wide maximum by DPP.
//   posterior_backward  the same loop downwards over the out-arcs.  b lives in LDS only; the a rows come back from the
//                       workspace PAHEAD frames ahead of use, every lane reading what it wrote itself.  Per frame: Z_t,
//                       gamma, and the 40 phoneme sums in an order that only the graph fixes (below).
#include "../../include/ppgs_amd.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <initializer_list>

namespace ppg {
int fail_message(int code, const char* fmt, ...);
// ppg_align.hip: the prepared frames (176 B per frame) and the check of the in-arc lists, one verdict per graph
void launch_align_prepare(void* stream, const float* ppg, int frames, int items, const int32_t* lengths, float* logp);
void launch_viterbi_check(void* stream, int graphs, int n_states, int n_arcs, int max_states,
                          const int32_t* state_begin, const int32_t* state_phonemes, const float* stay,
                          const float* initial, const float* final_, const int32_t* arc_begin, const int32_t* sources,
                          const float* weights, int32_t* verdict);
}

namespace {

// the prepared frame and its staging, as ppg_align.hip has them
constexpr int NP = 40;                        // phonemes
constexpr int PREP = 44;                      // floats per prepared frame: 40 log-posteriors, their maximum, 3 zeros
constexpr int PREP_VEC = PREP / 4;
constexpr int CHUNK = 32;                     // frames staged in LDS at a time
constexpr int CHUNK_VEC = CHUNK * PREP_VEC;
constexpr int FETCH = (CHUNK_VEC + 63) / 64;  // 16-byte pieces per lane and chunk

constexpr int PSTATES = PPG_VITERBI_MAX_STATES;
constexpr int PLEAD = 2;                      // arcs per state taken in lock step over a lane's slots
constexpr int PBATCH = 4;                     // arcs of a state read ahead of their exponentials, past the first two
constexpr int PHELD = 4096;                   // arcs of a graph a wave keeps in LDS (32 KiB) at most
constexpr int PAHEAD = 3;                     // frames the backward pass reads its rows of `a` ahead of their use
constexpr int PPOST = 64;                     // frames of `post` staged in LDS: 256 contiguous bytes per phoneme row
constexpr float LOG2E = 1.44269504088896340736f;
constexpr float LN2 = 0.69314718055994530942f;
static_assert(PSTATES % 256 == 0 && PPG_VITERBI_MAX_ARCS <= 1 << 15, "16 bits of arc index, 16 of degree");

struct PosteriorLayout {
    size_t logp, rows, shifts, verdict, bytes;                // byte offsets into the workspace
};

inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

// floats of one row of `a`: whole passes over the call's largest graph (ppg_viterbi's rounding of a back-pointer row)
__host__ __device__ inline int posterior_row(int max_states) {
    return max_states <= 64 ? 64 : (max_states + 255) & ~255;
}

// (65535 items of 65536 frames and 1024 states are 1.8e13 bytes: inside a size_t)
inline PosteriorLayout posterior_layout(int items, int frames, int max_states) {
    PosteriorLayout w{};
    const size_t slots = (size_t)items * frames;
    size_t at = 0;
    w.logp = at; at = align256(at + slots * PREP * sizeof(float));
    w.rows = at; at = align256(at + slots * posterior_row(max_states) * sizeof(float));
    w.shifts = at; at = align256(at + slots * sizeof(double));
    w.verdict = at; at = align256(at + (size_t)PPG_VITERBI_MAX_GRAPHS * sizeof(int));
    w.bytes = at;
    return w;
}

// a weight is finite or -inf
__device__ __forceinline__ bool bad_weight(float w) { return w != w || w == INFINITY; }

// grid (graphs), 64 threads, after viterbi_check: a graph it passed has its states inside the arrays, 1 .. max_states of
// them, and in-arc lists that rise inside their array.  Every test stands before the read that depends on it.
__global__ __launch_bounds__(64) void posterior_check(int n_arcs, const int* __restrict__ state_begin,
                                                       const int* __restrict__ arc_begin,
                                                       const int* __restrict__ out_begin,
                                                       const int* __restrict__ targets,
                                                       const float* __restrict__ out_weights, int* __restrict__ verdict)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    if (verdict[g] == 0) return;                               // (uniform)
    const int first = state_begin[g], end = state_begin[g + 1];
    const int S = end - first;
    bool bad = false;
    for (int n = first + lane; n < end; n += 64) {
        const int a0 = out_begin[n], a1 = out_begin[n + 1];    // (n + 1 <= n_states: the array has that entry)
        bool wrong = a0 < 0 || a1 > n_arcs || a1 < a0;
        if (!wrong)
            for (int j = a0; j < a1; ++j) wrong |= (unsigned)targets[j] >= (unsigned)S || bad_weight(out_weights[j]);
        bad |= wrong;
    }
    bool fine = !__any(bad);
    // (non-decreasing inside the graph and inside [0, n_arcs] by now) the transpose has the in-arcs' count
    if (fine) fine = out_begin[end] - out_begin[first] == arc_begin[end] - arc_begin[first];
    if (!fine && lane == 0) verdict[g] = 0;
}

// the prepared frames t0 .. t0 + CHUNK - 1 of one utterance, those below T only, one 16-byte piece per lane and u
__device__ __forceinline__ void fetch(const float4* __restrict__ src, int t0, int T, int lane, float4 (&piece)[FETCH]) {
    const int pieces = t0 < 0 ? 0 : min(CHUNK, T - t0) * PREP_VEC;     // <= 0 outside the utterance: nothing is read
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

// A wave-wide reduction by DPP in a fixed order: inside the quads, the rows of 16, then across the rows; the result is
// lane 63's, read as a scalar.  Call it from wave-uniform control flow.
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp(float v, float identity) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(v), CTRL, ROWS, 0xf,
                                                      false));
}
template <class Op>
__device__ __forceinline__ float wave_reduce(float v, float identity, Op op) {
    v = op(v, dpp<0xB1 /* quad_perm 1,0,3,2 */, 0xf>(v, identity));
    v = op(v, dpp<0x4E /* quad_perm 2,3,0,1 */, 0xf>(v, identity));
    v = op(v, dpp<0x141 /* row_half_mirror */, 0xf>(v, identity));
    v = op(v, dpp<0x140 /* row_mirror */, 0xf>(v, identity));
    v = op(v, dpp<0x142 /* row_bcast:15 */, 0xa>(v, identity));    // rows 1 and 3 take in rows 0 and 2
    v = op(v, dpp<0x143 /* row_bcast:31 */, 0xc>(v, identity));    // rows 2 and 3 take in row 1: lane 63 has all
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_max(float v) {
    return wave_reduce(v, -INFINITY, [](float a, float b) { return fmaxf(a, b); });
}
__device__ __forceinline__ float wave_sum(float v) {
    return wave_reduce(v, 0.f, [](float a, float b) { return a + b; });
}

// The arcs of one graph, the in-arcs for the forward pass and the out-arcs for the backward: Held from LDS, where a piece
// is (the state at the arc's other end, the weight's bits), else from the caller's arrays.  `i` counts from the graph's
// first arc.
template <bool Held>
struct PosteriorArcs {
    const uint2* held; const int* ends; const float* weights; int count;
    __device__ __forceinline__ void get(int i, int& other, float& weight) const {
        if (Held) {
            const uint2 piece = held[i];
            other = (int)piece.x; weight = __uint_as_float(piece.y);
        } else {
            other = ends[i]; weight = weights[i];
        }
    }
};

// What a wave keeps of a state in LDS: `arcs`, the first arc (counted from the graph's first, low 16 bits) and the
// degree (high 16 bits) of the list the pass walks, the weight of staying, and the phoneme.
struct PosteriorTable {
    uint32_t arcs[PSTATES];
    float stay[PSTATES];
    uint8_t sym[PSTATES];
};
__device__ __forceinline__ int first_arc(uint32_t arcs) { return (int)(arcs & 0xffffu); }
__device__ __forceinline__ int degree_of(uint32_t arcs) { return (int)(arcs >> 16); }

// One more candidate c of an LSE held as (top, sum): the largest so far and the sum of exp(candidate - top).  One
// exponential: of -|c - top|, or of -inf where c is -inf (never of a difference of two infinities).
__device__ __forceinline__ void take(float c, float& top, float& sum) {
    const bool up = c > top;
    const float gap = c == -INFINITY ? -INFINITY : -fabsf(c - top);
    const float e = __builtin_amdgcn_exp2f(gap * LOG2E);
    sum = up ? fmaf(sum, e, 1.f) : sum + e;
    top = up ? c : top;
}

// LSE(before[n] + stay[n], before[other] + w for every arc of state n's list, in list order) for the G neighbouring
// states n0 .. n0 + G - 1 of one lane.  G = 4 moves every per-state word as one 16-byte piece.  No predicated loads:
// where a state has no such arc, an arc of the graph stands in at weight -inf.  A lane may diverge inside; call it from
// wave-uniform control flow.
template <int G, bool Held>
__device__ __forceinline__ void lse_states(int n0, const PosteriorTable& table, const PosteriorArcs<Held>& arcs,
                                           const float* __restrict__ before, float (&out)[G])
{
    static_assert(G == 1 || G == 4, "a word or a 16-byte piece per lane");
    uint32_t list[G];
    float top[G], sum[G];
    if constexpr (G == 4) {
        const uint4 m = *reinterpret_cast<const uint4*>(table.arcs + n0);
        const float4 o = *reinterpret_cast<const float4*>(table.stay + n0);
        const float4 b = *reinterpret_cast<const float4*>(before + n0);
        list[0] = m.x; list[1] = m.y; list[2] = m.z; list[3] = m.w;
        top[0] = b.x + o.x; top[1] = b.y + o.y; top[2] = b.z + o.z; top[3] = b.w + o.w;
    } else {
        list[0] = table.arcs[n0];
        top[0] = before[n0] + table.stay[n0];
    }
#pragma unroll
    for (int k = 0; k < G; ++k) sum[k] = 1.f;                  // staying: exp(0)
    if (arcs.count > 0) {                                      // (uniform) arc 0 stands in where a state has none
#pragma unroll
        for (int j = 0; j < PLEAD; ++j) {                      // the first arcs of the G states in lock step
            int p[G]; float w[G];
#pragma unroll
            for (int k = 0; k < G; ++k) {
                const bool there = j < degree_of(list[k]);
                arcs.get(there ? first_arc(list[k]) + j : 0, p[k], w[k]);
                w[k] = there ? w[k] : -INFINITY;
            }
#pragma unroll
            for (int k = 0; k < G; ++k) take(before[p[k]] + w[k], top[k], sum[k]);
        }
#pragma unroll
        for (int k = 0; k < G; ++k) {                          // what lies beyond: state by state, PBATCH at a time
            const int at = first_arc(list[k]), degree = degree_of(list[k]);
            for (int j0 = PLEAD; j0 < degree; j0 += PBATCH) {
                int p[PBATCH]; float w[PBATCH];
#pragma unroll
                for (int u = 0; u < PBATCH; ++u) {             // (past the last arc the last one again, at -inf)
                    arcs.get(at + min(j0 + u, degree - 1), p[u], w[u]);
                    w[u] = j0 + u < degree ? w[u] : -INFINITY;
                }
#pragma unroll
                for (int u = 0; u < PBATCH; ++u) take(before[p[u]] + w[u], top[k], sum[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < G; ++k) out[k] = fmaf(LN2, __builtin_amdgcn_logf(sum[k]), top[k]);     // (sum >= 1)
}

// What both passes do first: whether item `item` is this launch's to run (its lengths and graph fine, its graph of G's
// size), and the graph.  `refused`: the item gets total = NaN from the G = 1 launch, which every call makes.
struct PosteriorItem {
    int T, first, S, covered;
};
template <int G>
__device__ __forceinline__ bool posterior_item(int item, int frames, const int* __restrict__ lengths, int graphs,
                                               const int* __restrict__ which, const int* __restrict__ verdict,
                                               const int* __restrict__ state_begin, PosteriorItem& it, bool& refused)
{
    it.T = lengths[item];
    const int g = which ? which[item] : 0;
    bool fine = it.T >= 1 && it.T <= frames && (unsigned)g < (unsigned)graphs;
    if (fine) fine = verdict[g] != 0;                          // (then 1 <= S <= max_states, inside the arrays)
    refused = !fine;
    if (!fine) return false;
    it.first = state_begin[g];
    it.S = state_begin[g + 1] - it.first;
    it.covered = (it.S + 64 * G - 1) / (64 * G) * (64 * G);    // whole passes: <= posterior_row(max_states)
    return (it.S <= 64) == (G == 1);
}

// the table of one graph for the lists that begin at `begin` (the graph's first state's entry), the arcs into LDS if
// they fit, and both rows at -inf; returns the arcs' count.  The caller's barrier follows.
template <int G>
__device__ __forceinline__ int load_graph(const PosteriorItem& it, int lane, const int* __restrict__ begin,
                                          const int* __restrict__ ends, const float* __restrict__ weights,
                                          const int* __restrict__ phonemes, const float* __restrict__ stay,
                                          PosteriorTable& table, uint2* __restrict__ held_arcs, int held,
                                          float (&rows)[2][PSTATES])
{
    const int arc0 = begin[0], count = begin[it.S] - arc0;
    for (int n = lane; n < it.covered; n += 64) {
        const bool state = n < it.S;
        // states at or above S run along on phoneme 0 without arcs, at -inf
        table.arcs[n] = state ? (uint32_t)(begin[n] - arc0) | (uint32_t)(begin[n + 1] - begin[n]) << 16 : 0u;
        table.stay[n] = state ? stay[it.first + n] : -INFINITY;
        table.sym[n] = state ? (uint8_t)phonemes[it.first + n] : 0;
        rows[0][n] = rows[1][n] = -INFINITY;
    }
    if (count <= held)
        for (int i = lane; i < count; i += 64)
            held_arcs[i] = make_uint2((uint32_t)ends[arc0 + i], __float_as_uint(weights[arc0 + i]));
    return count;
}

// the emissions of a lane's G states from the prepared frame `e`
template <int G>
__device__ __forceinline__ void emissions(const float* __restrict__ e, const PosteriorTable& table, int n0,
                                          float (&cur)[G]) {
    if constexpr (G == 4) {
        const uint32_t s = *reinterpret_cast<const uint32_t*>(table.sym + n0);
        cur[0] = e[s & 0xff]; cur[1] = e[(s >> 8) & 0xff]; cur[2] = e[(s >> 16) & 0xff]; cur[3] = e[s >> 24];
    } else {
        cur[0] = e[table.sym[n0]];
    }
}

template <int G>
__device__ __forceinline__ void put(float* __restrict__ to, const float (&v)[G]) {
    if constexpr (G == 4) *reinterpret_cast<float4*>(to) = make_float4(v[0], v[1], v[2], v[3]);
    else to[0] = v[0];
}
template <int G>
__device__ __forceinline__ void get(const float* __restrict__ from, float (&v)[G]) {
    if constexpr (G == 4) {
        const float4 f = *reinterpret_cast<const float4*>(from);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
        v[0] = from[0];
    }
}

// grid (items), 64 threads, `held` * 8 bytes of dynamic LDS.  `row` = posterior_row(max_states) floats per frame of
// `rows`.  An utterance whose length is
// impossible, whose `which` names no graph or whose graph was refused gets total = NaN, one without a path total = -inf,
// and neither anything else; every other its total, and the rows a[t, .] and shifts C[t] of its frames.
template <int G>
__global__ __launch_bounds__(64) void posterior_forward(const float* __restrict__ logp, int frames,
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
                                                         const float* __restrict__ weights, int held,
                                                         int row, float* __restrict__ rows,
                                                         double* __restrict__ shifts,
                                                         double* __restrict__ total)
{
    __shared__ float4 stage[2][CHUNK_VEC];
    __shared__ __attribute__((aligned(16))) float a[2][PSTATES];
    __shared__ __attribute__((aligned(16))) PosteriorTable table;
    extern __shared__ uint2 held_arcs[];
    const int item = blockIdx.x, lane = threadIdx.x;
    PosteriorItem it;
    bool refused;
    if (!posterior_item<G>(item, frames, lengths, graphs, which, verdict, state_begin, it, refused)) {     // (uniform)
        if (G == 1 && refused && lane == 0) total[item] = NAN;
        return;
    }
    const int T = it.T, S = it.S, first = it.first, covered = it.covered;
    const int* begin = arc_begin + first;
    const int arc0 = begin[0];
    const int count = load_graph<G>(it, lane, begin, sources, weights, phonemes, stay, table, held_arcs, held, a);
    const bool keep = count <= held;                           // (uniform)
    const PosteriorArcs<true> in_lds{held_arcs, nullptr, nullptr, count};
    const PosteriorArcs<false> in_memory{nullptr, sources + arc0, weights + arc0, count};
    const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
    float* out = rows + (size_t)item * frames * row;
    double* out_shifts = shifts + (size_t)item * frames;
    double shift = 0.;                                         // C[t]
    float before = 0.f;                                        // m[t-1]
    // the frame walk of viterbi_programme: the prepared frames through LDS CHUNK at a time, the next chunk in flight
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
            const float* last = a[(t & 1) ^ 1];
            float most = -INFINITY;
            for (int n0 = lane * G; n0 < covered; n0 += 64 * G) {  // (uniform: every lane takes every pass)
                float cur[G], v[G];
                emissions<G>(e + u * PREP, table, n0, cur);
                if (t == 0) {                                  // (uniform)
#pragma unroll
                    for (int k = 0; k < G; ++k) v[k] = cur[k] + (n0 + k < S ? initial[first + n0 + k] : -INFINITY);
                } else {
                    if (keep) lse_states<G, true>(n0, table, in_lds, last, v);
                    else lse_states<G, false>(n0, table, in_memory, last, v);
#pragma unroll
                    for (int k = 0; k < G; ++k) v[k] = cur[k] + (v[k] - before);
                }
#pragma unroll
                for (int k = 0; k < G; ++k) most = fmaxf(most, v[k]);
                put<G>(a[t & 1] + n0, v);
                put<G>(out + (size_t)t * row + n0, v);
            }
            if (lane == 0) out_shifts[t] = shift;
            before = wave_max(most);
            if (before == -INFINITY) {                         // (uniform) nothing is alive: no path
                if (lane == 0) total[item] = -INFINITY;
                return;
            }
            if (t + 1 < T) shift += (double)before;
            __syncthreads();                                   // frame t+1 reads what this frame wrote
        }
        stash(stage[buf ^ 1], lane, next);                     // its readers passed the barrier above
        __syncthreads();
    }
    // total = C[T-1] + LSE over n of (a[T-1, n] + final[n]): the maximum, then the sum, states n = lane, lane + 64, ...
    const float* end = a[(T - 1) & 1];
    float most = -INFINITY;
    for (int n = lane; n < S; n += 64) most = fmaxf(most, end[n] + final_[first + n]);
    most = wave_max(most);
    if (most == -INFINITY) {                                   // (uniform) no state may end the path
        if (lane == 0) total[item] = -INFINITY;
        return;
    }
    float sum = 0.f;
    for (int n = lane; n < S; n += 64) sum += __builtin_amdgcn_exp2f((end[n] + final_[first + n] - most) * LOG2E);
    sum = wave_sum(sum);
    if (lane == 0) total[item] = shift + (double)fmaf(LN2, __builtin_amdgcn_logf(sum), most);
}

// The phoneme sums of one frame in an order that only the graph fixes.  `order` lists the states by phoneme, ascending
// state inside a phoneme (a stable counting sort), `from[p]` is where phoneme p's begin in it.  Lane l adds up the
// `span` = ceil(S / 64) positions from l * span on, starting anew where the phoneme changes, and leaves every running
// sum in a slot of its own; lane p < 40 then adds, lane by lane, the last sum of every lane that holds some of
// phoneme p.  On a graph whose states all carry one phoneme that is `span` + 64 additions in a row instead of S.
struct PosteriorOrder {
    uint16_t order[PSTATES];
    int from[NP + 1];
};

__device__ __forceinline__ void sort_states(const PosteriorTable& table, int S, int lane, PosteriorOrder& by) {
    int at = 0;                                                // (uniform) positions given out so far
    for (int p = 0; p < NP; ++p) {
        if (lane == 0) by.from[p] = at;
        for (int n0 = 0; n0 < S; n0 += 64) {
            const int n = n0 + lane;
            const bool mine = n < S && table.sym[n] == p;
            const unsigned long long votes = __ballot(mine);
            if (mine) by.order[at + __popcll(votes & ((1ull << lane) - 1))] = (uint16_t)n;
            at += __popcll(votes);
        }
    }
    if (lane == 0) by.from[NP] = at;                           // = S
}

// grid (items), 64 threads, `held` * 8 bytes of dynamic LDS.  Only the items the forward pass gave a finite total.
// `post` (items, 40, frames); `occupancy`
// NULL or (items, frames, state_stride).
template <int G>
__global__ __launch_bounds__(64) void posterior_backward(const float* __restrict__ logp, int frames,
                                                          const int* __restrict__ lengths, int graphs,
                                                          const int* __restrict__ which,
                                                          const int* __restrict__ verdict,
                                                          const int* __restrict__ state_begin,
                                                          const int* __restrict__ phonemes,
                                                          const float* __restrict__ stay,
                                                          const float* __restrict__ final_,
                                                          const int* __restrict__ out_begin,
                                                          const int* __restrict__ targets,
                                                          const float* __restrict__ out_weights, int held,
                                                          int row, const float* __restrict__ rows,
                                                          const double* __restrict__ total, float* __restrict__ post,
                                                          float* __restrict__ occupancy, int state_stride)
{
    constexpr int PASSES = G == 1 ? 1 : PSTATES / 256;
    __shared__ float4 stage[CHUNK_VEC];
    __shared__ __attribute__((aligned(16))) float eb[2][PSTATES];  // e + b of a frame; the older one serves as `run`
    __shared__ __attribute__((aligned(16))) float ab[PSTATES];     // b, then a + b, then exp(a + b - its maximum)
    __shared__ __attribute__((aligned(16))) PosteriorTable table;
    __shared__ PosteriorOrder by;
    __shared__ float sums[NP][PPOST];
    extern __shared__ uint2 held_arcs[];
    const int item = blockIdx.x, lane = threadIdx.x;
    PosteriorItem it;
    bool refused;
    if (!posterior_item<G>(item, frames, lengths, graphs, which, verdict, state_begin, it, refused)) return;   // (uniform)
    const double whole = total[item];
    if (!(whole > -INFINITY)) return;                          // (uniform) no path: nothing is written
    const int T = it.T, S = it.S, first = it.first, covered = it.covered;
    const int* begin = out_begin + first;
    const int arc0 = begin[0];
    const int count = load_graph<G>(it, lane, begin, targets, out_weights, phonemes, stay, table, held_arcs, held,
                                    eb);
    const bool keep = count <= held;                           // (uniform)
    __syncthreads();
    sort_states(table, S, lane, by);
    __syncthreads();
    const PosteriorArcs<true> in_lds{held_arcs, nullptr, nullptr, count};
    const PosteriorArcs<false> in_memory{nullptr, targets + arc0, out_weights + arc0, count};
    const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
    const float* in = rows + (size_t)item * frames * row;
    float* out = post + (size_t)item * NP * frames;
    float* out_states = occupancy ? occupancy + (size_t)item * frames * state_stride : nullptr;
    // the lane's sorted positions stay in registers for the whole utterance: the state, and whether it goes on with the
    // phoneme of the position before it in this lane; their running sums stand in `run` at lane * SPAN + u
    constexpr int SPAN = G == 1 ? 1 : PSTATES / 64, GOES_ON = 1 << 15;
    static_assert(PSTATES <= GOES_ON, "a state below its flag");
    const int span = (S + 63) / 64;                            // sorted positions per lane: <= SPAN
    int mine[SPAN];
#pragma unroll
    for (int u = 0; u < SPAN; ++u) {
        const int i = lane * span + u;
        const bool there = u < span && i < S;
        const int n = there ? by.order[i] : 0;
        const bool goes_on = there && u > 0 && table.sym[n] == table.sym[by.order[i - 1]];
        mine[u] = n | (goes_on ? GOES_ON : 0);                // (one that is not there: state 0, into a slot nobody reads)
    }
    // the lane's own states of row t, pass by pass, as the forward pass wrote them; nothing below frame 0
    float ahead[PAHEAD][PASSES][G];
    auto load_row = [&](int t, float (&to)[PASSES][G]) {
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int n0 = (p * 64 + lane) * G;
            if (t >= 0 && n0 < covered) get<G>(in + (size_t)t * row + n0, to[p]);     // (uniform)
            else
#pragma unroll
                for (int k = 0; k < G; ++k) to[p][k] = -INFINITY;
        }
    };
#pragma unroll
    for (int d = 0; d < PAHEAD; ++d) load_row(T - 1 - d, ahead[d]);
    float4 next[FETCH];
    int c = (T - 1) / CHUNK;                                   // the chunk of prepared frames in `stage`
    fetch(src, c * CHUNK, T, lane, next);
    stash(stage, lane, next);
    __syncthreads();
    fetch(src, (c - 1) * CHUNK, T, lane, next);
    float before = 0.f;                                        // the maximum of b[t+1, .]
    for (int t = T - 1; t >= 0; --t) {
        const float* e = reinterpret_cast<const float*>(stage) + (t - c * CHUNK) * PREP;
        const float* last = eb[(t & 1) ^ 1];
        float* now = eb[t & 1];
        float most = -INFINITY;
        for (int n0 = lane * G; n0 < covered; n0 += 64 * G) {  // (uniform: every lane takes every pass)
            float cur[G], v[G];
            emissions<G>(e, table, n0, cur);
            if (t == T - 1) {                                  // (uniform)
#pragma unroll
                for (int k = 0; k < G; ++k) v[k] = n0 + k < S ? final_[first + n0 + k] : -INFINITY;
            } else {
                if (keep) lse_states<G, true>(n0, table, in_lds, last, v);
                else lse_states<G, false>(n0, table, in_memory, last, v);
#pragma unroll
                for (int k = 0; k < G; ++k) v[k] -= before;
            }
#pragma unroll
            for (int k = 0; k < G; ++k) most = fmaxf(most, v[k]);
            put<G>(ab + n0, v);
#pragma unroll
            for (int k = 0; k < G; ++k) v[k] += cur[k];
            put<G>(now + n0, v);
        }
        before = wave_max(most);                               // (finite: a path exists)
        // a + b from the row read ahead (every lane touches only what it wrote), and its maximum
        float peak = -INFINITY;
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int n0 = (p * 64 + lane) * G;
            if (n0 < covered) {                                // (uniform)
                float v[G];
                get<G>(ab + n0, v);
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    v[k] += ahead[0][p][k];
                    peak = fmaxf(peak, v[k]);
                }
                put<G>(ab + n0, v);
            }
        }
#pragma unroll
        for (int d = 0; d + 1 < PAHEAD; ++d)
#pragma unroll
            for (int p = 0; p < PASSES; ++p)
#pragma unroll
                for (int k = 0; k < G; ++k) ahead[d][p][k] = ahead[d + 1][p][k];
        load_row(t - PAHEAD, ahead[PAHEAD - 1]);
        peak = wave_max(peak);
        peak = peak > -INFINITY ? peak : 0.f;                  // (a path exists, so it is finite: no NaN if it were not)
        float sum = 0.f;
        for (int n0 = lane * G; n0 < covered; n0 += 64 * G) {
            float v[G];
            get<G>(ab + n0, v);
#pragma unroll
            for (int k = 0; k < G; ++k) {
                v[k] = __builtin_amdgcn_exp2f((v[k] - peak) * LOG2E);
                sum += v[k];
            }
            put<G>(ab + n0, v);
        }
        sum = wave_sum(sum);
        const float scale = sum > 0.f ? 1.f / sum : 0.f;
        if (out_states) {
            float* to = out_states + (size_t)t * state_stride;
            for (int n0 = lane * G; n0 < covered; n0 += 64 * G) {
                float v[G];
                get<G>(ab + n0, v);
#pragma unroll
                for (int k = 0; k < G; ++k)
                    if (n0 + k < S) to[n0 + k] = v[k] * scale;
            }
        }
        __syncthreads();                                       // ab stands; `last` has been read by every lane
        float* run = eb[(t & 1) ^ 1];
        {
            float x[SPAN];
#pragma unroll
            for (int u = 0; u < SPAN; ++u) x[u] = ab[mine[u] & (PSTATES - 1)];     // (all in flight together)
            float sofar = 0.f;
#pragma unroll
            for (int u = 0; u < SPAN; ++u) {                   // (no masks: a lane's SPAN slots are its own)
                sofar = fmaf(sofar, (float)((mine[u] >> 15) & 1), x[u]);
                run[lane * SPAN + u] = sofar;
            }
        }
        __syncthreads();
        if (lane < NP) {
            const int i0 = by.from[lane], i1 = by.from[lane + 1];
            float whole_sum = 0.f;
            if (i1 > i0)
                for (int l = i0 / span; l <= (i1 - 1) / span; ++l)
                    whole_sum += run[l * SPAN + min(span, i1 - l * span) - 1];
            sums[lane][t % PPOST] = whole_sum * scale;
        }
        __syncthreads();                                       // frame t-1 writes where `run` stood
        if (t % PPOST == 0) {                                  // (uniform) frames t .. t + 63 stand: whole rows of them
            if (t + lane < T)
#pragma unroll 8
                for (int p = 0; p < NP; ++p) out[(size_t)p * frames + t + lane] = sums[p][lane];
        }
        if (t == c * CHUNK && t > 0) {                         // (uniform) the chunk below, which has been in flight
            stash(stage, lane, next);
            __syncthreads();
            --c;
            fetch(src, (c - 1) * CHUNK, T, lane, next);
        }
    }
}

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

bool posterior_sizes_fine(int items, int frames, int max_states) {
    return items > 0 && items <= PPG_VITERBI_MAX_ITEMS && frames > 0 && frames <= PPG_POSTERIOR_MAX_FRAMES &&
           max_states > 0 && max_states <= PPG_VITERBI_MAX_STATES;
}

}  // namespace

extern "C" {

size_t ppg_posterior_workspace_bytes(int items, int frames, int max_states) {
    return posterior_sizes_fine(items, frames, max_states) ? posterior_layout(items, frames, max_states).bytes : 0;
}

int ppg_posterior(int device, const float* ppg, int frames, int items, const int32_t* lengths, int graphs, int n_states,
                  int n_arcs, int max_states, const int32_t* state_begin, const int32_t* state_phonemes,
                  const float* stay, const float* initial, const float* final_, const int32_t* arc_begin,
                  const int32_t* sources, const float* weights, const int32_t* out_begin, const int32_t* targets,
                  const float* out_weights, const int32_t* which, double* total, float* post, float* occupancy,
                  int state_stride, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ppg || !lengths || items <= 0 || frames <= 0) return ppg::fail_message(PPG_EINVAL, "posterior: bad argument");
    if (frames > PPG_POSTERIOR_MAX_FRAMES)
        return ppg::fail_message(PPG_EINVAL, "posterior: %d frames, at most %d", frames, PPG_POSTERIOR_MAX_FRAMES);
    if (items > PPG_VITERBI_MAX_ITEMS)
        return ppg::fail_message(PPG_EINVAL, "posterior: %d items, at most %d per call", items, PPG_VITERBI_MAX_ITEMS);
    if (!workspace || graphs <= 0 || max_states <= 0 || n_arcs < 0)
        return ppg::fail_message(PPG_EINVAL, "posterior: bad argument");
    if (graphs > PPG_VITERBI_MAX_GRAPHS)
        return ppg::fail_message(PPG_EINVAL, "posterior: %d graphs, at most %d per call", graphs,
                                 PPG_VITERBI_MAX_GRAPHS);
    if (max_states > PPG_VITERBI_MAX_STATES)
        return ppg::fail_message(PPG_EINVAL, "posterior: %d states, at most %d per graph", max_states,
                                 PPG_VITERBI_MAX_STATES);
    if (n_states < graphs || (long long)n_states > (long long)graphs * max_states ||
        (long long)n_arcs > (long long)graphs * PPG_VITERBI_MAX_ARCS)
        return ppg::fail_message(PPG_EINVAL, "posterior: %d states and %d arcs cannot be %d graphs of 1 to %d states "
                                 "and at most %d arcs", n_states, n_arcs, graphs, max_states, PPG_VITERBI_MAX_ARCS);
    if (n_arcs > 0 && (!sources || !weights || !targets || !out_weights))
        return ppg::fail_message(PPG_EINVAL, "posterior: bad argument");
    if (occupancy && state_stride < max_states)
        return ppg::fail_message(PPG_EINVAL, "posterior: a state stride of %d for graphs of up to %d states",
                                 state_stride, max_states);
    if (const int rc = check_words("posterior", {ppg, lengths, state_begin, state_phonemes, stay, initial, final_,
                                                 arc_begin, out_begin, post},
                                   {sources, weights, targets, out_weights, which, occupancy}))
        return rc;
    if (!total || reinterpret_cast<uintptr_t>(total) % 8)
        return ppg::fail_message(PPG_EINVAL, "posterior: total must be float64, 8-byte aligned");
    const PosteriorLayout w = posterior_layout(items, frames, max_states);
    if (workspace_bytes < w.bytes)
        return ppg::fail_message(PPG_EINVAL, "posterior: workspace of %zu bytes, %zu needed", workspace_bytes, w.bytes);
    if (reinterpret_cast<uintptr_t>(workspace) % 16)
        return ppg::fail_message(PPG_EINVAL, "posterior: workspace must be 16-byte aligned");
    if (hipSetDevice(device) != hipSuccess)
        return ppg::fail_message(PPG_EDEVICE, "no HIP device: the post-ops have no CPU path");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    float* logp = reinterpret_cast<float*>(ws + w.logp);
    float* rows = reinterpret_cast<float*>(ws + w.rows);
    double* shifts = reinterpret_cast<double*>(ws + w.shifts);
    int* verdict = reinterpret_cast<int*>(ws + w.verdict);
    const int row = posterior_row(max_states);
    // the arcs a wave keeps in LDS, sized by the call as in ppg_viterbi, so that small graphs leave a CU's LDS to more
    // waves.  A full block beside the backward pass's 40 KiB of static LDS is more than the 64 KiB a launch gets
    // without asking.
    const int held = n_arcs < PHELD ? n_arcs : PHELD;
    const size_t lds = (size_t)held * sizeof(uint2);
    for (const void* kernel : {reinterpret_cast<const void*>(posterior_backward<1>),
                               reinterpret_cast<const void*>(posterior_backward<4>)})
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PHELD * (int)sizeof(uint2)) !=
            hipSuccess)
            return ppg::fail_message(PPG_EDEVICE, "posterior: the device refuses %d bytes of dynamic LDS",
                                     PHELD * (int)sizeof(uint2));
    ppg::launch_align_prepare(stream, ppg, frames, items, lengths, logp);
    ppg::launch_viterbi_check(stream, graphs, n_states, n_arcs, max_states, state_begin, state_phonemes, stay, initial,
                              final_, arc_begin, sources, weights, verdict);
    hipLaunchKernelGGL(posterior_check, dim3(graphs), dim3(64), 0, s, n_arcs, state_begin, arc_begin, out_begin,
                       targets, out_weights, verdict);
    // the graphs of at most 64 states, then, if the call may hold any, the larger ones: an item runs in one of the two
    hipLaunchKernelGGL(posterior_forward<1>, dim3(items), dim3(64), lds, s, logp, frames, lengths, graphs, which,
                       verdict, state_begin, state_phonemes, stay, initial, final_, arc_begin, sources, weights, held,
                       row, rows, shifts, total);
    if (row > 64)
        hipLaunchKernelGGL(posterior_forward<4>, dim3(items), dim3(64), lds, s, logp, frames, lengths, graphs, which,
                           verdict, state_begin, state_phonemes, stay, initial, final_, arc_begin, sources, weights,
                           held, row, rows, shifts, total);
    hipLaunchKernelGGL(posterior_backward<1>, dim3(items), dim3(64), lds, s, logp, frames, lengths, graphs, which,
                       verdict, state_begin, state_phonemes, stay, final_, out_begin, targets, out_weights, held, row,
                       rows, total, post, occupancy, state_stride);
    if (row > 64)
        hipLaunchKernelGGL(posterior_backward<4>, dim3(items), dim3(64), lds, s, logp, frames, lengths, graphs, which,
                           verdict, state_begin, state_phonemes, stay, final_, out_begin, targets, out_weights, held,
                           row, rows, total, post, occupancy, state_stride);
    const hipError_t he = hipGetLastError();
    return he == hipSuccess ? PPG_OK : ppg::fail_message(PPG_EDEVICE, "posterior: %s", hipGetErrorString(he));
}

}  // extern "C"
