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

// ---- fixed-lag posteriors on a live stream (ppg_posterior_stream_*) ----
//
// The two passes above carried across the pushes of a stream.  A stream has a position p (frames received), an emission
// point c, a block H and a lag L.  The forward pass is posterior_forward's from absolute frame 0: the row a[p-1] (in the
// ring), its maximum m[p-1] and the float64 shift C[p-1] are the state, so every row has the bits posterior_forward
// writes for the whole recording, whatever the pushes.  Block k = frames [kH, (k+1)H) is given out by the first push
// after which p >= (k+1)H + L: a backward pass from the horizon h = (k+1)H + L - 1 with beta = 0 for every state (an
// open end: `final` is not read), beta alone down to the block's last frame, posterior_backward's whole step over the
// block.  What is given out is columns [kH, (k+1)H) of ppg_posterior(ppg[:, :h+1], the graph with final = 0), bit for
// bit.  The flush is one backward pass from p - 1 under the graph's own `final` down to c.
// The caller owns the state: four blocks, each 256-byte aligned: the heads (40 B per stream), the ring of rows of `a`
// (posterior_row(max_states) floats per frame, slot t % W), the ring of prepared frames (176 B per frame) and one
// verdict per graph (room for as many graphs as streams).  One wave per stream; G = 1 and G = 4 launches as above, each
// taking the streams whose own graph is of its size, so a stream's bits never depend on its neighbours.
//   posterior_stream_reset     opens (graph, H, L per stream from the verdicts) or restarts streams
//   posterior_stream_forward   copies the push's prepared frames into the ring, walks the forward over them into the
//                              ring, leaves evidence = C[p-1] + LSE(a[p-1]) and the new head
//   posterior_stream_backward  the blocks the push completed, a workgroup each; or, as the flush, the rest under `final`
//   posterior_stream_total     what a flush says of every stream: count, begin and total

struct PosteriorHead {
    int position, previous;                   // p, and p before the last push: c = posterior_emitted(p) at all times
    int graph;                                // the stream's graph; -1: refused or missing when the stream was opened
    int block, lag;                           // H and L
    int dead;                                 // a frame left no state alive: nothing more is taken
    float before;                             // m[p-1]
    int spare;
    double shift;                             // C[p-1]
};
static_assert(sizeof(PosteriorHead) == 40, "the head is 40 bytes");

struct PosteriorStreamLayout {
    size_t heads, rows, kept, verdict, bytes;                  // byte offsets into the state
};

// (65535 streams of 65536 frames and 1024 states are 1.8e13 bytes: inside a size_t)
inline PosteriorStreamLayout posterior_stream_layout(int streams, int window, int max_states) {
    PosteriorStreamLayout w{};
    const size_t slots = (size_t)streams * window;
    size_t at = 0;
    w.heads = at; at = align256(at + (size_t)streams * sizeof(PosteriorHead));
    w.rows = at; at = align256(at + slots * posterior_row(max_states) * sizeof(float));
    w.kept = at; at = align256(at + slots * PREP * sizeof(float));
    w.verdict = at; at = align256(at + (size_t)streams * sizeof(int));
    w.bytes = at;
    return w;
}

// c after p frames: the blocks whose horizon has been received
__host__ __device__ inline long long posterior_emitted(long long p, int block, int lag) {
    return p < lag ? 0 : (p - lag) / block * block;
}

// The first frame of the `index`-th block that a push from `previous` to `received` frames completes, or -1 if it
// completes fewer: in 64 bits, since index * block passes 2^31 for arguments the entries accept.
__host__ __device__ inline long long posterior_block(long long previous, long long received, int block, int lag,
                                                     long long index) {
    const long long c = posterior_emitted(previous, block, lag), stop = posterior_emitted(received, block, lag);
    return index >= 0 && index < (stop - c) / block ? c + index * block : -1;
}

// The graph of a stream from the caller's arrays, S inside [1, row] whatever they hold; whether it is of G's size.
template <int G>
__device__ __forceinline__ bool stream_graph(int g, int row, const int* __restrict__ state_begin, PosteriorItem& it) {
    it.T = 0;
    it.first = state_begin[g];
    it.S = min(max(state_begin[g + 1] - it.first, 1), row);
    it.covered = (it.S + 64 * G - 1) / (64 * G) * (64 * G);
    return (it.S <= 64) == (G == 1);
}

__device__ __forceinline__ void restart(PosteriorHead* head) {
    head->position = 0; head->previous = 0; head->dead = 0; head->before = 0.f; head->spare = 0; head->shift = 0.;
}

// grid (ceil(streams / 64)), 64 threads: thread = stream.  Open: stream i starts at frame 0 with graph which[i] (null:
// graph 0), or with none (-1) if that names no graph or the graph was refused.  Else the streams `which` flags (null:
// all) start again and keep their graph, H and L.
template <bool Open>
__global__ __launch_bounds__(64) void posterior_stream_reset(int streams, const int* __restrict__ which, int graphs,
                                                              const int* __restrict__ verdict, int block, int lag,
                                                              PosteriorHead* __restrict__ heads)
{
    const int item = blockIdx.x * 64 + threadIdx.x;
    if (item >= streams) return;
    if (Open) {
        const int g = which ? which[item] : 0;
        const bool fine = (unsigned)g < (unsigned)graphs && verdict[g] != 0;
        heads[item].graph = fine ? g : -1;
        heads[item].block = block;
        heads[item].lag = lag;
    } else if (which && which[item] == 0) {
        return;
    }
    restart(heads + item);
}

// LSE over n of (end[n] + final_[n]) (final_ null: + 0) in posterior_forward's order: the maximum, then the sum, states
// n = lane, lane + 64, ...  False where no state may end.  Call it from wave-uniform control flow.
__device__ __forceinline__ bool lse_end(const float* __restrict__ end, const float* __restrict__ final_, int S, int lane,
                                        float& out) {
    float most = -INFINITY;
    for (int n = lane; n < S; n += 64) most = fmaxf(most, end[n] + (final_ ? final_[n] : 0.f));
    most = wave_max(most);
    if (most == -INFINITY) return false;                       // (uniform)
    float sum = 0.f;
    for (int n = lane; n < S; n += 64)
        sum += __builtin_amdgcn_exp2f((end[n] + (final_ ? final_[n] : 0.f) - most) * LOG2E);
    sum = wave_sum(sum);
    out = fmaf(LN2, __builtin_amdgcn_logf(sum), most);
    return true;
}

// The prepared frames [t0, t0 + CHUNK) of a stream's ring that lie in [lo, hi), one 16-byte piece per lane and u.  t0 is
// a multiple of CHUNK and the window one of 2 * CHUNK, so a chunk never wraps.
__device__ __forceinline__ void fetch_ring(const float4* __restrict__ ring, int window, int t0, int lo, int hi, int lane,
                                           float4 (&piece)[FETCH]) {
    const int slot0 = t0 >= 0 ? t0 % window : 0;
#pragma unroll
    for (int u = 0; u < FETCH; ++u) {
        const int idx = u * 64 + lane;
        const int f = t0 + idx / PREP_VEC;
        const bool there = idx < CHUNK_VEC && f >= lo && f < hi;
        piece[u] = there ? ring[(size_t)slot0 * PREP_VEC + idx] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// grid (streams), 64 threads, `held` * 8 bytes of dynamic LDS.  logp (streams, frames, 44) are the push's prepared
// frames.  A stream without a graph gets count = -1 from the G = 1 launch, which every push makes; one that cannot take
// its frames count = -1 too, and keeps its state; a dead one count = 0 and evidence = -inf; every other count = 0, which
// posterior_stream_backward replaces if a block completed, and its evidence.
template <int G>
__global__ __launch_bounds__(64) void posterior_stream_forward(const float* __restrict__ logp, int frames,
                                                                const int* __restrict__ lengths, int window,
                                                                PosteriorHead* __restrict__ heads,
                                                                const int* __restrict__ state_begin,
                                                                const int* __restrict__ phonemes,
                                                                const float* __restrict__ stay,
                                                                const float* __restrict__ initial,
                                                                const int* __restrict__ arc_begin,
                                                                const int* __restrict__ sources,
                                                                const float* __restrict__ weights, int held, int row,
                                                                float* __restrict__ rows, float4* __restrict__ kept,
                                                                int* __restrict__ begin_out, int* __restrict__ count,
                                                                double* __restrict__ evidence)
{
    __shared__ float4 stage[2][CHUNK_VEC];
    __shared__ __attribute__((aligned(16))) float a[2][PSTATES];
    __shared__ __attribute__((aligned(16))) PosteriorTable table;
    extern __shared__ uint2 held_arcs[];
    const int item = blockIdx.x, lane = threadIdx.x;
    const PosteriorHead head = heads[item];
    if (head.graph < 0) {                                      // (uniform)
        if (G == 1 && lane == 0) {
            begin_out[item] = 0; count[item] = -1; evidence[item] = NAN;
        }
        return;
    }
    PosteriorItem it;
    if (!stream_graph<G>(head.graph, row, state_begin, it)) return;    // (uniform) the other launch's
    const int T = lengths[item], p = head.position, c = (int)posterior_emitted(p, head.block, head.lag);
    const bool takes = T >= 0 && T <= frames && T <= INT32_MAX - p && T <= window - (p - c);
    if (head.dead || !takes) {                                 // (uniform)
        if (lane == 0) {
            heads[item].previous = p;                          // no block completes
            begin_out[item] = c;
            count[item] = head.dead ? 0 : -1;
            evidence[item] = head.dead ? (double)-INFINITY : (double)NAN;
        }
        return;
    }
    const int S = it.S, first = it.first, covered = it.covered;
    const int* begin = arc_begin + first;
    const int arc0 = begin[0];
    const int arcs = load_graph<G>(it, lane, begin, sources, weights, phonemes, stay, table, held_arcs, held, a);
    const bool keep = arcs <= held;                            // (uniform)
    const PosteriorArcs<true> in_lds{held_arcs, nullptr, nullptr, arcs};
    const PosteriorArcs<false> in_memory{nullptr, sources + arc0, weights + arc0, arcs};
    const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
    float4* ring = kept + (size_t)item * window * PREP_VEC;
    float* out = rows + (size_t)item * window * row;
    int slot = p % window;                                     // of frame t
    for (int idx = lane; idx < T * PREP_VEC; idx += 64) {      // T <= window: a slot wraps once at most
        int to = slot + idx / PREP_VEC;
        to = to >= window ? to - window : to;
        ring[(size_t)to * PREP_VEC + idx % PREP_VEC] = src[idx];
    }
    __syncthreads();                                           // the rows stand at -inf
    if (p > 0) {                                               // a[p-1], every lane the pieces it wrote
        const float* from = out + (size_t)(slot == 0 ? window - 1 : slot - 1) * row;
        for (int n0 = lane * G; n0 < covered; n0 += 64 * G) {
            float v[G];
            get<G>(from + n0, v);
            put<G>(a[(p - 1) & 1] + n0, v);
        }
    }
    double shift = head.shift;                                 // C[t-1], then C[t]
    float before = head.before;                                // m[t-1]
    float4 next[FETCH];
    fetch(src, 0, T, lane, next);
    stash(stage[0], lane, next);
    __syncthreads();
    int buf = 0;
    for (int r0 = 0; r0 < T; r0 += CHUNK, buf ^= 1) {
        fetch(src, r0 + CHUNK, T, lane, next);
        const float* e = reinterpret_cast<const float*>(stage[buf]);
        const int chunk = min(CHUNK, T - r0);
        for (int u = 0; u < chunk; ++u) {
            const int t = p + r0 + u;
            const float* last = a[(t & 1) ^ 1];
            if (t > 0) shift += (double)before;
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
                put<G>(out + (size_t)slot * row + n0, v);
            }
            slot = slot + 1 == window ? 0 : slot + 1;
            before = wave_max(most);
            if (before == -INFINITY) {                         // (uniform) nothing is alive: the stream is dead
                if (lane == 0) {
                    heads[item].dead = 1;
                    heads[item].previous = p;
                    begin_out[item] = c; count[item] = 0; evidence[item] = (double)-INFINITY;
                }
                return;
            }
            __syncthreads();                                   // frame t+1 reads what this frame wrote
        }
        stash(stage[buf ^ 1], lane, next);                     // its readers passed the barrier above
        __syncthreads();
    }
    float lse = 0.f;
    if (p + T > 0) lse_end(a[(p + T - 1) & 1], nullptr, S, lane, lse);     // (uniform; alive, so there is one)
    if (lane == 0) {
        heads[item].position = p + T;
        heads[item].previous = p;
        heads[item].before = before;
        heads[item].shift = shift;
        begin_out[item] = c; count[item] = 0;
        evidence[item] = p + T > 0 ? shift + (double)lse : 0.;
    }
}

// grid (streams), 64 threads: what a flush says of every stream, before posterior_stream_backward gives the frames out
// and posterior_stream_reset starts the streams again.  A stream `which` leaves out (null: none), one without a graph
// or one that has received nothing: count = 0, total = NaN; a dead one, or one in which no alive state may end: count =
// 0, total = -inf; every other count = p - c and total = C[p-1] + LSE over n of (a[p-1, n] + final[n]) as
// posterior_forward adds it up.
__global__ __launch_bounds__(64) void posterior_stream_total(int window, const int* __restrict__ which,
                                                              const PosteriorHead* __restrict__ heads,
                                                              const int* __restrict__ state_begin,
                                                              const float* __restrict__ final_, int row,
                                                              const float* __restrict__ rows,
                                                              int* __restrict__ begin_out, int* __restrict__ count,
                                                              double* __restrict__ total)
{
    const int item = blockIdx.x, lane = threadIdx.x;
    const PosteriorHead head = heads[item];
    const int p = head.position;
    const bool meant = head.graph >= 0 && !(which && which[item] == 0) && p > 0;
    if (!meant || head.dead) {                                 // (uniform)
        if (lane == 0) {
            begin_out[item] = head.graph < 0 ? 0 : (int)posterior_emitted(p, head.block, head.lag);
            count[item] = 0;
            total[item] = meant ? (double)-INFINITY : (double)NAN;
        }
        return;
    }
    PosteriorItem it;
    stream_graph<1>(head.graph, row, state_begin, it);
    const int c = (int)posterior_emitted(p, head.block, head.lag);
    float lse = 0.f;
    const bool ends = lse_end(rows + ((size_t)item * window + (p - 1) % window) * row, final_ + it.first, it.S, lane,
                              lse);
    if (lane == 0) {
        begin_out[item] = c;
        count[item] = ends ? p - c : 0;
        total[item] = ends ? head.shift + (double)lse : (double)-INFINITY;
    }
}

// grid (blocks, streams), 64 threads, `held` * 8 bytes of dynamic LDS, after posterior_stream_forward.  Workgroup
// (k, i) runs the k-th of the blocks that stream i's push completed, if there are so many (a push of F frames completes
// at most F): the blocks of a push read the rings and nothing of each other.  `post` (streams, 40, cap), `occupancy`
// NULL or (streams, cap, state_stride): column j is frame begin + j, columns at or past cap or count are never written.
// Flush (grid (1, streams)), after posterior_stream_total: the streams it left a count for give out [c, p) under
// `final_`.
template <int G, bool Flush>
__global__ __launch_bounds__(64) void posterior_stream_backward(int window,
                                                                 const PosteriorHead* __restrict__ heads,
                                                                 const int* __restrict__ state_begin,
                                                                 const int* __restrict__ phonemes,
                                                                 const float* __restrict__ stay,
                                                                 const float* __restrict__ final_,
                                                                 const int* __restrict__ out_begin,
                                                                 const int* __restrict__ targets,
                                                                 const float* __restrict__ out_weights, int held,
                                                                 int row, const float* __restrict__ rows,
                                                                 const float4* __restrict__ kept, int cap,
                                                                 float* __restrict__ post,
                                                                 float* __restrict__ occupancy, int state_stride,
                                                                 int* __restrict__ count)
{
    constexpr int PASSES = G == 1 ? 1 : PSTATES / 256;
    __shared__ float4 stage[CHUNK_VEC];
    __shared__ __attribute__((aligned(16))) float eb[2][PSTATES];  // e + b of a frame; the older one serves as `run`
    __shared__ __attribute__((aligned(16))) float ab[PSTATES];     // b, then a + b, then exp(a + b - its maximum)
    __shared__ __attribute__((aligned(16))) PosteriorTable table;
    __shared__ PosteriorOrder by;
    __shared__ float sums[NP][PPOST];
    extern __shared__ uint2 held_arcs[];
    const int item = blockIdx.y, lane = threadIdx.x;
    const PosteriorHead head = heads[item];
    if (head.graph < 0 || head.dead) return;                   // (uniform)
    PosteriorItem it;
    if (!stream_graph<G>(head.graph, row, state_begin, it)) return;    // (uniform) the other launch's
    const int p = head.position;
    const int S = it.S, first = it.first, covered = it.covered;
    const float* in = rows + (size_t)item * window * row;
    int c, lo, top, h;                        // column 0; the frames [lo, top] are given out from the horizon h < p
    if (Flush) {
        if (count[item] <= 0) return;                          // (uniform) posterior_stream_total: nothing to give out
        c = lo = (int)posterior_emitted(p, head.block, head.lag);
        top = h = p - 1;
    } else {
        c = (int)posterior_emitted(head.previous, head.block, head.lag);
        const int stop = (int)posterior_emitted(p, head.block, head.lag);
        const long long mine = posterior_block(head.previous, p, head.block, head.lag, blockIdx.x);
        if (mine < 0) return;                                  // (uniform) the push completed fewer blocks
        lo = (int)mine;                                        // (< stop <= p: what follows stays inside an int)
        top = lo + head.block - 1;
        h = top + head.lag;
        if (blockIdx.x == 0 && lane == 0) count[item] = stop - c;
    }
    const int* begin = out_begin + first;
    const int arc0 = begin[0];
    const int arcs = load_graph<G>(it, lane, begin, targets, out_weights, phonemes, stay, table, held_arcs, held, eb);
    const bool keep = arcs <= held;                            // (uniform)
    __syncthreads();
    sort_states(table, S, lane, by);
    // b at the horizon: the graph's own `final` at the flush, else an open end
    for (int n0 = lane * G; n0 < covered; n0 += 64 * G) {
        float v[G];
#pragma unroll
        for (int k = 0; k < G; ++k) v[k] = n0 + k < S ? (Flush ? final_[first + n0 + k] : 0.f) : -INFINITY;
        put<G>(ab + n0, v);
    }
    __syncthreads();
    const PosteriorArcs<true> in_lds{held_arcs, nullptr, nullptr, arcs};
    const PosteriorArcs<false> in_memory{nullptr, targets + arc0, out_weights + arc0, arcs};
    const float4* ring = kept + (size_t)item * window * PREP_VEC;
    float* out = post + (size_t)item * NP * cap;
    float* out_states = occupancy ? occupancy + (size_t)item * cap * state_stride : nullptr;
    // the lane's sorted positions, as posterior_backward keeps them
    constexpr int SPAN = G == 1 ? 1 : PSTATES / 64, GOES_ON = 1 << 15;
    const int span = (S + 63) / 64;                            // sorted positions per lane: <= SPAN
    int mine[SPAN];
#pragma unroll
    for (int u = 0; u < SPAN; ++u) {
        const int i = lane * span + u;
        const bool there = u < span && i < S;
        const int n = there ? by.order[i] : 0;
        const bool goes_on = there && u > 0 && table.sym[n] == table.sym[by.order[i - 1]];
        mine[u] = n | (goes_on ? GOES_ON : 0);
    }
    // the lane's own states of a row of `a`, pass by pass, as the forward pass wrote them: the rows from `top` down, one
    // per call; nothing below the block
    float ahead[PAHEAD][PASSES][G];
    int behind = top % window, left = top - lo + 1;            // the slot of the next row to read; rows left
    auto load_row = [&](float (&to)[PASSES][G]) {
#pragma unroll
        for (int q = 0; q < PASSES; ++q) {
            const int n0 = (q * 64 + lane) * G;
            if (left > 0 && n0 < covered) get<G>(in + (size_t)behind * row + n0, to[q]);      // (uniform)
            else
#pragma unroll
                for (int k = 0; k < G; ++k) to[q][k] = -INFINITY;
        }
        behind = behind == 0 ? window - 1 : behind - 1;
        --left;
    };
#pragma unroll
    for (int d = 0; d < PAHEAD; ++d) load_row(ahead[d]);
    float4 next[FETCH];
    int cidx = h / CHUNK;                                      // the chunk of prepared frames in `stage`
    fetch_ring(ring, window, cidx * CHUNK, lo, h + 1, lane, next);
    stash(stage, lane, next);
    __syncthreads();
    fetch_ring(ring, window, (cidx - 1) * CHUNK, lo, h + 1, lane, next);
    float before = 0.f;                                        // the maximum of b[t+1, .]
    for (int t = h; t >= lo; --t) {
        const bool whole = t <= top;                           // (uniform) a frame of the block: the full step
        const float* e = reinterpret_cast<const float*>(stage) + (t - cidx * CHUNK) * PREP;
        const float* last = eb[(t & 1) ^ 1];
        float* now = eb[t & 1];
        float most = -INFINITY;
        for (int n0 = lane * G; n0 < covered; n0 += 64 * G) {  // (uniform: every lane takes every pass)
            float cur[G], v[G];
            emissions<G>(e, table, n0, cur);
            if (t == h) {                                      // (uniform) b at the horizon, every lane what it wrote
                get<G>(ab + n0, v);
            } else {
                if (keep) lse_states<G, true>(n0, table, in_lds, last, v);
                else lse_states<G, false>(n0, table, in_memory, last, v);
#pragma unroll
                for (int k = 0; k < G; ++k) v[k] -= before;
            }
#pragma unroll
            for (int k = 0; k < G; ++k) most = fmaxf(most, v[k]);
            if (whole) put<G>(ab + n0, v);
#pragma unroll
            for (int k = 0; k < G; ++k) v[k] += cur[k];
            put<G>(now + n0, v);
        }
        before = wave_max(most);                               // (finite: a path exists)
        if (whole) {
            const int j = t - c;                               // the column
            // a + b from the row read ahead (every lane touches only what it wrote), and its maximum
            float peak = -INFINITY;
#pragma unroll
            for (int q = 0; q < PASSES; ++q) {
                const int n0 = (q * 64 + lane) * G;
                if (n0 < covered) {                            // (uniform)
                    float v[G];
                    get<G>(ab + n0, v);
#pragma unroll
                    for (int k = 0; k < G; ++k) {
                        v[k] += ahead[0][q][k];
                        peak = fmaxf(peak, v[k]);
                    }
                    put<G>(ab + n0, v);
                }
            }
#pragma unroll
            for (int d = 0; d + 1 < PAHEAD; ++d)
#pragma unroll
                for (int q = 0; q < PASSES; ++q)
#pragma unroll
                    for (int k = 0; k < G; ++k) ahead[d][q][k] = ahead[d + 1][q][k];
            load_row(ahead[PAHEAD - 1]);
            peak = wave_max(peak);
            peak = peak > -INFINITY ? peak : 0.f;              // (a path exists, so it is finite: no NaN if it were not)
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
            if (out_states && j < cap) {                       // (uniform)
                float* to = out_states + (size_t)j * state_stride;
                for (int n0 = lane * G; n0 < covered; n0 += 64 * G) {
                    float v[G];
                    get<G>(ab + n0, v);
#pragma unroll
                    for (int k = 0; k < G; ++k)
                        if (n0 + k < S) to[n0 + k] = v[k] * scale;
                }
            }
            __syncthreads();                                   // ab stands; `last` has been read by every lane
            float* run = eb[(t & 1) ^ 1];
            {
                float x[SPAN];
#pragma unroll
                for (int u = 0; u < SPAN; ++u) x[u] = ab[mine[u] & (PSTATES - 1)];     // (all in flight together)
                float sofar = 0.f;
#pragma unroll
                for (int u = 0; u < SPAN; ++u) {               // (no masks: a lane's SPAN slots are its own)
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
                sums[lane][j % PPOST] = whole_sum * scale;
            }
            __syncthreads();                                   // frame t-1 writes where `run` stood
            if (j % PPOST == 0 || t == lo) {                   // (uniform) the columns from j on stand, 64 at most
                const int column = j + lane;
                if (column <= min(j | (PPOST - 1), top - c) && column < cap)
#pragma unroll 8
                    for (int q = 0; q < NP; ++q) out[(size_t)q * cap + column] = sums[q][column % PPOST];
            }
        } else {
            __syncthreads();                                   // frame t-1 reads `now` and writes `last`
        }
        if (t == cidx * CHUNK && t > lo) {                     // (uniform) the chunk below, which has been in flight
            stash(stage, lane, next);
            __syncthreads();
            --cidx;
            fetch_ring(ring, window, (cidx - 1) * CHUNK, lo, h + 1, lane, next);
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

bool posterior_stream_sizes_fine(int streams, int window, int max_states) {
    return streams > 0 && streams <= PPG_VITERBI_STREAM_MAX_STREAMS && window >= PPG_VITERBI_STREAM_MIN_WINDOW &&
           window <= PPG_VITERBI_STREAM_MAX_WINDOW && window % 64 == 0 && max_states > 0 &&
           max_states <= PPG_VITERBI_MAX_STATES;
}

// the checks every entry of the live posterior shares: the state and its geometry
int check_posterior_stream_state(const char* what, const void* state, int streams, int window, int max_states) {
    if (!state) return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    if (!posterior_stream_sizes_fine(streams, window, max_states))
        return ppg::fail_message(PPG_EINVAL, "%s: %d streams of a window of %d frames and %d states: 1 to %d streams, a "
                                 "window that is a multiple of 64 from %d to %d, 1 to %d states", what, streams, window,
                                 max_states, PPG_VITERBI_STREAM_MAX_STREAMS, PPG_VITERBI_STREAM_MIN_WINDOW,
                                 PPG_VITERBI_STREAM_MAX_WINDOW, PPG_VITERBI_MAX_STATES);
    if (reinterpret_cast<uintptr_t>(state) % 16)
        return ppg::fail_message(PPG_EINVAL, "%s: the state must be 16-byte aligned", what);
    return PPG_OK;
}

// the packed graphs of a live posterior: as ppg_posterior takes them, and no more graphs than streams
int check_posterior_stream_graphs(const char* what, int streams, int graphs, int n_states, int n_arcs, int max_states,
                                  const void* sources, const void* weights, const void* targets,
                                  const void* out_weights) {
    if (graphs <= 0 || n_states <= 0 || n_arcs < 0) return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    if (graphs > streams)
        return ppg::fail_message(PPG_EINVAL, "%s: %d graphs for %d streams, at most one each", what, graphs, streams);
    if (n_states < graphs || (long long)n_states > (long long)graphs * max_states ||
        (long long)n_arcs > (long long)graphs * PPG_VITERBI_MAX_ARCS)
        return ppg::fail_message(PPG_EINVAL, "%s: %d states and %d arcs cannot be %d graphs of 1 to %d states and at "
                                 "most %d arcs", what, n_states, n_arcs, graphs, max_states, PPG_VITERBI_MAX_ARCS);
    if (n_arcs > 0 && (!sources || !weights || !targets || !out_weights))
        return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    return PPG_OK;
}

// the outputs a push and a flush share
int check_posterior_stream_outputs(const char* what, int cap, const void* occupancy, int state_stride, int max_states,
                                   const void* float64) {
    if (cap < 1) return ppg::fail_message(PPG_EINVAL, "%s: cap = %d, must be at least 1", what, cap);
    if (occupancy && state_stride < max_states)
        return ppg::fail_message(PPG_EINVAL, "%s: a state stride of %d for graphs of up to %d states", what,
                                 state_stride, max_states);
    if (!float64 || reinterpret_cast<uintptr_t>(float64) % 8)
        return ppg::fail_message(PPG_EINVAL, "%s: evidence and total must be float64, 8-byte aligned", what);
    return PPG_OK;
}

// the arcs a wave keeps in LDS beside the backward pass's static 40 KiB: more than a launch gets without asking
template <bool Flush>
int allow_posterior_stream_lds(const char* what) {
    for (const void* kernel : {reinterpret_cast<const void*>(posterior_stream_backward<1, Flush>),
                               reinterpret_cast<const void*>(posterior_stream_backward<4, Flush>)})
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PHELD * (int)sizeof(uint2)) !=
            hipSuccess)
            return ppg::fail_message(PPG_EDEVICE, "%s: the device refuses %d bytes of dynamic LDS", what,
                                     PHELD * (int)sizeof(uint2));
    return PPG_OK;
}

int posterior_stream_launched(const char* what) {
    const hipError_t he = hipGetLastError();
    return he == hipSuccess ? PPG_OK : ppg::fail_message(PPG_EDEVICE, "%s: %s", what, hipGetErrorString(he));
}

}  // namespace

extern "C" {

int64_t ppg_posterior_stream_emitted(int64_t received, int block, int lag) {
    if (received < 0 || block < 1 || lag < 0) return -1;
    return posterior_emitted(received, block, lag);
}

int64_t ppg_posterior_stream_block(int64_t previous, int64_t received, int block, int lag, int64_t index) {
    if (previous < 0 || received < previous || block < 1 || lag < 0) return -1;
    return posterior_block(previous, received, block, lag, index);
}

size_t ppg_posterior_stream_state_bytes(int streams, int window, int max_states) {
    return posterior_stream_sizes_fine(streams, window, max_states)
               ? posterior_stream_layout(streams, window, max_states).bytes : 0;
}

size_t ppg_posterior_stream_workspace_bytes(int streams, int frames) {
    if (streams <= 0 || streams > PPG_VITERBI_STREAM_MAX_STREAMS || frames <= 0 ||
        frames > PPG_VITERBI_STREAM_MAX_WINDOW)
        return 0;
    return align256((size_t)streams * frames * PREP * sizeof(float));
}

int ppg_posterior_stream_open(int device, void* state, int streams, int window, int graphs, int n_states, int n_arcs,
                              int max_states, const int32_t* state_begin, const int32_t* state_phonemes,
                              const float* stay, const float* initial, const float* final_, const int32_t* arc_begin,
                              const int32_t* sources, const float* weights, const int32_t* out_begin,
                              const int32_t* targets, const float* out_weights, const int32_t* which_graph, int block,
                              int lag, void* stream) {
    const char* what = "posterior_stream_open";
    if (const int rc = check_posterior_stream_state(what, state, streams, window, max_states)) return rc;
    if (const int rc = check_posterior_stream_graphs(what, streams, graphs, n_states, n_arcs, max_states, sources,
                                                     weights, targets, out_weights))
        return rc;
    if (block < 1 || lag < 0 || (long long)block + lag > window)
        return ppg::fail_message(PPG_EINVAL, "%s: block = %d and lag = %d: a block of at least 1 frame, a lag of at "
                                 "least 0, together at most the window of %d", what, block, lag, window);
    if (const int rc = check_words(what, {state_begin, state_phonemes, stay, initial, final_, arc_begin, out_begin},
                                   {sources, weights, targets, out_weights, which_graph}))
        return rc;
    if (hipSetDevice(device) != hipSuccess)
        return ppg::fail_message(PPG_EDEVICE, "no HIP device: the post-ops have no CPU path");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const PosteriorStreamLayout w = posterior_stream_layout(streams, window, max_states);
    char* st = static_cast<char*>(state);
    int* verdict = reinterpret_cast<int*>(st + w.verdict);
    ppg::launch_viterbi_check(stream, graphs, n_states, n_arcs, max_states, state_begin, state_phonemes, stay, initial,
                              final_, arc_begin, sources, weights, verdict);
    hipLaunchKernelGGL(posterior_check, dim3(graphs), dim3(64), 0, s, n_arcs, state_begin, arc_begin, out_begin,
                       targets, out_weights, verdict);
    hipLaunchKernelGGL(posterior_stream_reset<true>, dim3((streams + 63) / 64), dim3(64), 0, s, streams, which_graph,
                       graphs, verdict, block, lag, reinterpret_cast<PosteriorHead*>(st + w.heads));
    return posterior_stream_launched(what);
}

int ppg_posterior_stream_reset(int device, void* state, int streams, int window, int max_states, const int32_t* which,
                               void* stream) {
    const char* what = "posterior_stream_reset";
    if (const int rc = check_posterior_stream_state(what, state, streams, window, max_states)) return rc;
    if (const int rc = check_words(what, {}, {which})) return rc;
    if (hipSetDevice(device) != hipSuccess)
        return ppg::fail_message(PPG_EDEVICE, "no HIP device: the post-ops have no CPU path");
    const PosteriorStreamLayout w = posterior_stream_layout(streams, window, max_states);
    char* st = static_cast<char*>(state);
    hipLaunchKernelGGL(posterior_stream_reset<false>, dim3((streams + 63) / 64), dim3(64), 0,
                       static_cast<hipStream_t>(stream), streams, which, 0, static_cast<const int*>(nullptr), 0, 0,
                       reinterpret_cast<PosteriorHead*>(st + w.heads));
    return posterior_stream_launched(what);
}

int ppg_posterior_stream_push(int device, void* state, int streams, int window, const float* ppg, int frames,
                              const int32_t* lengths, int graphs, int n_states, int n_arcs, int max_states,
                              const int32_t* state_begin, const int32_t* state_phonemes, const float* stay,
                              const float* initial, const float* final_, const int32_t* arc_begin,
                              const int32_t* sources, const float* weights, const int32_t* out_begin,
                              const int32_t* targets, const float* out_weights, int cap, float* post, float* occupancy,
                              int state_stride, int32_t* begin, int32_t* count, double* evidence, void* workspace,
                              size_t workspace_bytes, void* stream) {
    const char* what = "posterior_stream_push";
    if (const int rc = check_posterior_stream_state(what, state, streams, window, max_states)) return rc;
    if (const int rc = check_posterior_stream_graphs(what, streams, graphs, n_states, n_arcs, max_states, sources,
                                                     weights, targets, out_weights))
        return rc;
    if (const int rc = check_words(what, {ppg, lengths, state_begin, state_phonemes, stay, initial, final_, arc_begin,
                                          out_begin, post, begin, count, workspace},
                                   {sources, weights, targets, out_weights, occupancy}))
        return rc;
    if (frames < 1 || frames > PPG_VITERBI_STREAM_MAX_WINDOW)
        return ppg::fail_message(PPG_EINVAL, "%s: %d frames, must be 1 .. %d", what, frames,
                                 PPG_VITERBI_STREAM_MAX_WINDOW);
    if ((long long)frames * streams > PPG_POSTERIOR_STREAM_MAX_PUSH)  // a workgroup per frame and stream: one launch
        return ppg::fail_message(PPG_EINVAL, "%s: %d frames for %d streams, at most %d frames x streams a push", what,
                                 frames, streams, PPG_POSTERIOR_STREAM_MAX_PUSH);
    if (const int rc = check_posterior_stream_outputs(what, cap, occupancy, state_stride, max_states, evidence))
        return rc;
    const size_t need = align256((size_t)streams * frames * PREP * sizeof(float));
    if (workspace_bytes < need)
        return ppg::fail_message(PPG_EINVAL, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 16)
        return ppg::fail_message(PPG_EINVAL, "%s: workspace must be 16-byte aligned", what);
    if (hipSetDevice(device) != hipSuccess)
        return ppg::fail_message(PPG_EDEVICE, "no HIP device: the post-ops have no CPU path");
    if (const int rc = allow_posterior_stream_lds<false>(what)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const PosteriorStreamLayout w = posterior_stream_layout(streams, window, max_states);
    char* st = static_cast<char*>(state);
    PosteriorHead* heads = reinterpret_cast<PosteriorHead*>(st + w.heads);
    float* rows = reinterpret_cast<float*>(st + w.rows);
    float4* kept = reinterpret_cast<float4*>(st + w.kept);
    float* logp = static_cast<float*>(workspace);
    const int row = posterior_row(max_states);
    const int held = n_arcs < PHELD ? n_arcs : PHELD;         // the arcs a wave keeps in LDS, sized by the call
    const size_t lds = (size_t)held * sizeof(uint2);
    ppg::launch_align_prepare(stream, ppg, frames, streams, lengths, logp);
    // the streams whose graph has at most 64 states, then, if the state may hold any, the larger ones
    hipLaunchKernelGGL(posterior_stream_forward<1>, dim3(streams), dim3(64), lds, s, logp, frames, lengths, window,
                       heads, state_begin, state_phonemes, stay, initial, arc_begin, sources, weights, held, row, rows,
                       kept, begin, count, evidence);
    if (row > 64)
        hipLaunchKernelGGL(posterior_stream_forward<4>, dim3(streams), dim3(64), lds, s, logp, frames, lengths, window,
                           heads, state_begin, state_phonemes, stay, initial, arc_begin, sources, weights, held, row,
                           rows, kept, begin, count, evidence);
    // a push of `frames` frames completes at most as many blocks: a workgroup each, most of which leave at once
    hipLaunchKernelGGL((posterior_stream_backward<1, false>), dim3(frames, streams), dim3(64), lds, s, window, heads,
                       state_begin, state_phonemes, stay, final_, out_begin, targets, out_weights, held, row, rows, kept,
                       cap, post, occupancy, state_stride, count);
    if (row > 64)
        hipLaunchKernelGGL((posterior_stream_backward<4, false>), dim3(frames, streams), dim3(64), lds, s, window,
                           heads, state_begin, state_phonemes, stay, final_, out_begin, targets, out_weights, held, row,
                           rows, kept, cap, post, occupancy, state_stride, count);
    return posterior_stream_launched(what);
}

int ppg_posterior_stream_flush(int device, void* state, int streams, int window, int graphs, int n_states, int n_arcs,
                               int max_states, const int32_t* state_begin, const int32_t* state_phonemes,
                               const float* stay, const float* initial, const float* final_, const int32_t* arc_begin,
                               const int32_t* sources, const float* weights, const int32_t* out_begin,
                               const int32_t* targets, const float* out_weights, const int32_t* which, int cap,
                               float* post, float* occupancy, int state_stride, int32_t* begin, int32_t* count,
                               double* total, void* stream) {
    const char* what = "posterior_stream_flush";
    if (const int rc = check_posterior_stream_state(what, state, streams, window, max_states)) return rc;
    if (const int rc = check_posterior_stream_graphs(what, streams, graphs, n_states, n_arcs, max_states, sources,
                                                     weights, targets, out_weights))
        return rc;
    if (const int rc = check_words(what, {state_begin, state_phonemes, stay, initial, final_, arc_begin, out_begin, post,
                                          begin, count},
                                   {sources, weights, targets, out_weights, which, occupancy}))
        return rc;
    if (const int rc = check_posterior_stream_outputs(what, cap, occupancy, state_stride, max_states, total)) return rc;
    if (hipSetDevice(device) != hipSuccess)
        return ppg::fail_message(PPG_EDEVICE, "no HIP device: the post-ops have no CPU path");
    if (const int rc = allow_posterior_stream_lds<true>(what)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const PosteriorStreamLayout w = posterior_stream_layout(streams, window, max_states);
    char* st = static_cast<char*>(state);
    PosteriorHead* heads = reinterpret_cast<PosteriorHead*>(st + w.heads);
    const float* rows = reinterpret_cast<const float*>(st + w.rows);
    const float4* kept = reinterpret_cast<const float4*>(st + w.kept);
    const int row = posterior_row(max_states);
    const int held = n_arcs < PHELD ? n_arcs : PHELD;
    const size_t lds = (size_t)held * sizeof(uint2);
    hipLaunchKernelGGL(posterior_stream_total, dim3(streams), dim3(64), 0, s, window, which, heads, state_begin, final_,
                       row, rows, begin, count, total);
    hipLaunchKernelGGL((posterior_stream_backward<1, true>), dim3(1, streams), dim3(64), lds, s, window, heads,
                       state_begin, state_phonemes, stay, final_, out_begin, targets, out_weights, held, row, rows, kept,
                       cap, post, occupancy, state_stride, count);
    if (row > 64)
        hipLaunchKernelGGL((posterior_stream_backward<4, true>), dim3(1, streams), dim3(64), lds, s, window, heads,
                           state_begin, state_phonemes, stay, final_, out_begin, targets, out_weights, held, row, rows,
                           kept, cap, post, occupancy, state_stride, count);
    hipLaunchKernelGGL(posterior_stream_reset<false>, dim3((streams + 63) / 64), dim3(64), 0, s, streams, which, 0,
                       static_cast<const int*>(nullptr), 0, 0, heads);
    return posterior_stream_launched(what);
}

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
