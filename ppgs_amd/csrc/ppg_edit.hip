// Phoneme error rate: the weighted edit distance of two phoneme sequences, with the alignment as edit operations, on
// the device.  The discrete sibling of ppg_dtw.hip: the same skewed wavefront, a table look-up for a cost.
//
//   D[0, 0] = 0, (N + 1) x (M + 1) cells in fp32; for every other cell, in this order of preference,
//     diagonal   D[i-1, j-1] + sub[r[i-1], h[j-1]]
//     deletion   D[i-1, j]   + del[r[i-1]]
//     insertion  D[i, j-1]   + ins[h[j-1]]
//   each ONE fp32 add; a candidate outside the table does not exist; a later candidate replaces an earlier one only
//   if it is strictly smaller (comparisons only).  Row 0 and column 0 are therefore sequential sums.
//
// Two kernels on one stream, no allocation, no synchronisation:
//   edit_programme  one wave per pair, no barrier.  Rows come in blocks of 256 = 64 lanes x 4 table rows
//                   (i = 256 b + 4 l + k + 1); lane l meets table column j = s - l at step s, column 0 included, so
//                   column 0 falls out of the same rule (its diagonal and left neighbours are +inf).  The lane keeps
//                   its 4 reference tokens, their deletion costs and its 4 cells of the previous column in registers;
//                   the row above, the hypothesis token and its insertion cost come down from lane l - 1 by a
//                   cross-lane move; lane 0 is fed 64 columns at a time -- row 0, summed in order, for the first
//                   block and the last row of the previous block, through LDS, for the others.  The substitution,
//                   deletion and insertion counts ride beside the cost (S | D << 16: H and I follow from N and M), so
//                   a call without ops writes nothing per cell.  With ops it stores one direction byte per cell.
//   edit_traceback  one thread per pair; K = H + S + D + I is known, so the operations are written in forward order,
//                   and the corpus statistics are accumulated with 64-bit integer atomics.
#include "../../include/ppgs_amd.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace ppg {
int fail_message(int code, const char* fmt, ...);
}

namespace {

constexpr int NP = 40;            // phonemes
constexpr int STRIP = 4;          // rows per lane
constexpr int BLOCK_ROWS = 64 * STRIP;
constexpr int CHUNK = 8;          // steps per unrolled group of the programme
constexpr int STATS = (NP + 1) * (NP + 1);   // the (41, 41) table; then the counters: pairs, invalid pairs

struct Layout {
    size_t valid, dirs, bytes;    // byte offsets into the workspace; dirs == 0: none
    int blocks, steps;            // row blocks per pair, steps per block in the direction table
};

inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

inline Layout layout(int pairs, int tokens_ref, int tokens_hyp, int want_ops) {
    Layout w{};
    w.blocks = (tokens_ref + BLOCK_ROWS - 1) / BLOCK_ROWS;
    w.steps = tokens_hyp + 64;                                  // columns 0 .. M, plus the skew of 63 lanes
    size_t at = 0;
    w.valid = at; at = align256(at + (size_t)pairs * sizeof(int));
    if (want_ops) { w.dirs = at; at = align256(at + (size_t)pairs * w.blocks * w.steps * 64 * sizeof(uint32_t)); }
    w.bytes = at;
    return w;
}

// lane l <- lane l - 1; lane 0 <- first
__device__ __forceinline__ int lane_up(int v, int first) {
    return __builtin_amdgcn_update_dpp(first, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ float lane_up(float v, float first) {
    return __int_as_float(lane_up(__float_as_int(v), __float_as_int(first)));
}
__device__ __forceinline__ float read_lane(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// 64 more cells of row 0, one per lane: the running sum takes the insertion costs one at a time, in order
__device__ __forceinline__ float row0(float& sum, float ins_cost, int lane) {
    float mine = 0.f;
#pragma unroll 8
    for (int c = 0; c < 64; ++c) {
        sum = sum + read_lane(ins_cost, c);
        mine = lane == c ? sum : mine;
    }
    return mine;
}

// grid (pairs), 64 threads; dynamic LDS: (tokens_hyp + 1) x (float + int), the last row of the previous block
template <bool kOps>
__global__ __launch_bounds__(64) void edit_programme(const int* __restrict__ ref, int tokens_ref,
                                                      const int* __restrict__ hyp, int tokens_hyp,
                                                      const int* __restrict__ len_ref, const int* __restrict__ len_hyp,
                                                      const float* __restrict__ sub, const float* __restrict__ del,
                                                      const float* __restrict__ ins, int blocks, int steps,
                                                      float* __restrict__ total, int* __restrict__ counts,
                                                      int* __restrict__ valid, uint32_t* __restrict__ dirs)
{
    __shared__ float s_sub[NP * NP];
    __shared__ float s_del[NP], s_ins[NP];
    extern __shared__ float edge[];
    float* edge_d = edge;
    int* edge_n = reinterpret_cast<int*>(edge + tokens_hyp + 1);
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int raw_n = len_ref[pair], raw_m = len_hyp[pair];
    const int tn = min(raw_n, tokens_ref), tm = min(raw_m, tokens_hyp);
    const int* r_src = ref + (size_t)pair * tokens_ref;
    const int* h_src = hyp + (size_t)pair * tokens_hyp;
    for (int i = lane; i < NP * NP; i += 64) s_sub[i] = sub ? sub[i] : (i / NP == i % NP ? 0.f : 1.f);
    if (lane < NP) { s_del[lane] = del ? del[lane] : 1.f; s_ins[lane] = ins ? ins[lane] : 1.f; }
    __syncthreads();                                           // the only one: from here on the wave runs in lockstep
    bool bad = raw_n < 0 || raw_m < 0;
    for (int i = lane; i < tn; i += 64) bad |= (unsigned)r_src[i] >= (unsigned)NP;
    for (int j = lane; j < tm; j += 64) bad |= (unsigned)h_src[j] >= (unsigned)NP;
    if (__ballot(bad)) {                                       // not a pair (uniform)
        if (lane < 4) counts[pair * 4 + lane] = 0;
        if (lane == 0) { total[pair] = NAN; valid[pair] = 0; }
        return;
    }
    const float inf = INFINITY;
    const int used = (tn + BLOCK_ROWS - 1) / BLOCK_ROWS;
    float d[STRIP]; int n[STRIP];
    float sum = 0.f;                                           // row 0 so far
    if (used == 0) {                                           // an empty reference: row 0 is the table
        for (int s0 = 0; s0 <= tm; s0 += 64) {
            const int col = s0 + lane;
            const bool real = col >= 1 && col <= tm;
            const int token = real ? h_src[col - 1] : 0;
            (void)row0(sum, real ? s_ins[token] : 0.f, lane);
        }
        if (lane == 0) {
            total[pair] = sum; valid[pair] = 1;
            counts[pair * 4 + 0] = 0; counts[pair * 4 + 1] = 0; counts[pair * 4 + 2] = 0; counts[pair * 4 + 3] = tm;
        }
        return;
    }
    for (int block = 0; block < used; ++block) {
        const int rows = min(tn - block * BLOCK_ROWS, BLOCK_ROWS);
        const int lanes = (rows + STRIP - 1) / STRIP;
        const int nsteps = tm + lanes;                         // columns 0 .. M for every lane of the block
        const bool hand_on = block + 1 < used;                 // then rows == BLOCK_ROWS and lane 63 holds the last row
        uint32_t* dst = kOps ? dirs + ((size_t)pair * blocks + block) * steps * 64 + lane : nullptr;
        int rt[STRIP]; float rd[STRIP];                        // the strip's reference tokens and their deletion costs
#pragma unroll
        for (int k = 0; k < STRIP; ++k) {
            const int a = block * BLOCK_ROWS + lane * STRIP + k;
            rt[k] = a < tn ? r_src[a] : 0;                     // rows past N are computed and never read
            rd[k] = s_del[rt[k]];
            rt[k] *= NP;
            d[k] = inf; n[k] = 0;
        }
        float diag_d = inf; int diag_n = 0;                    // the cell above-left: none at column 0
        float top_d = inf; int top_n = 0;                      // 64 columns of the row above the block, one per lane
        int feed_h = 0; float feed_i = 0.f;                    // 64 columns of the hypothesis: token and insertion cost
        int hv = 0; float iv = 0.f;                            // the lane's column
        for (int s0 = 0; s0 < nsteps; s0 += CHUNK) {
            if ((s0 & 63) == 0) {
                const int col = s0 + lane;
                const bool real = col >= 1 && col <= tm;
                feed_h = real ? h_src[col - 1] : 0;
                feed_i = real ? s_ins[feed_h] : 0.f;
                if (block == 0) {
                    top_d = row0(sum, feed_i, lane);
                } else {
                    top_d = col <= tm ? edge_d[col] : inf;
                    top_n = col <= tm ? edge_n[col] : 0;
                }
            }
#pragma unroll
            for (int u = 0; u < CHUNK; ++u) {
                const int s = s0 + u;
                const float first_d = read_lane(top_d, s & 63);
                const int first_n = __builtin_amdgcn_readlane(top_n, s & 63);
                const int first_h = __builtin_amdgcn_readlane(feed_h, s & 63);
                const float first_i = read_lane(feed_i, s & 63);
                const float up_d = lane_up(d[STRIP - 1], first_d);
                const int up_n = lane_up(n[STRIP - 1], first_n);
                hv = lane_up(hv, first_h);
                iv = lane_up(iv, first_i);
                const int j = s - lane;
                if (j >= 0 && j <= tm && lane < lanes) {
                    float pd = diag_d, qd = up_d; int pn = diag_n, qn = up_n;     // diagonal and upper neighbour of row k
                    uint32_t code = 0;
#pragma unroll
                    for (int k = 0; k < STRIP; ++k) {
                        const float old_d = d[k]; const int old_n = n[k];
                        float best = pd + s_sub[rt[k] + hv];
                        int cnt = pn + (rt[k] != hv * NP);
                        uint32_t dir = 0;
                        const float gone = qd + rd[k];
                        if (gone < best) { best = gone; cnt = qn + 0x10000; dir = 1; }
                        const float come = old_d + iv;
                        if (come < best) { best = come; cnt = old_n; dir = 2; }
                        d[k] = best; n[k] = cnt;
                        code |= dir << (8 * k);
                        pd = old_d; pn = old_n; qd = best; qn = cnt;
                    }
                    if (kOps) dst[(size_t)s * 64] = code;
                    if (hand_on && lane == 63) { edge_d[j] = d[STRIP - 1]; edge_n[j] = n[STRIP - 1]; }
                }
                diag_d = up_d; diag_n = up_n;
            }
        }
    }
    const int last = tn - 1 - (used - 1) * BLOCK_ROWS;         // row of the final cell inside the last block
    if (lane == last / STRIP) {
        const int k = last % STRIP;
        float rd = d[0]; int rn = n[0];
#pragma unroll
        for (int q = 1; q < STRIP; ++q) { rd = k == q ? d[q] : rd; rn = k == q ? n[q] : rn; }
        const int subs = rn & 0xffff, dels = rn >> 16, hits = tn - subs - dels;
        total[pair] = rd;
        valid[pair] = 1;
        counts[pair * 4 + 0] = hits; counts[pair * 4 + 1] = subs; counts[pair * 4 + 2] = dels;
        counts[pair * 4 + 3] = tm - hits - subs;
    }
}

// grid (ceil(pairs / 64)), 64 threads: thread = pair
__global__ __launch_bounds__(64) void edit_traceback(const uint32_t* __restrict__ dirs, const int* __restrict__ valid,
                                                      const int* __restrict__ counts, int pairs,
                                                      const int* __restrict__ ref, int tokens_ref,
                                                      const int* __restrict__ hyp, int tokens_hyp,
                                                      const int* __restrict__ len_ref, const int* __restrict__ len_hyp,
                                                      int blocks, int steps, int* __restrict__ ops,
                                                      int* __restrict__ ops_length,
                                                      unsigned long long* __restrict__ statistics)
{
    const int pair = blockIdx.x * 64 + threadIdx.x;
    if (pair >= pairs) return;
    if (!valid[pair]) {
        ops_length[pair] = 0;
        if (statistics) atomicAdd(statistics + STATS + 1, 1ull);
        return;
    }
    const int* c = counts + pair * 4;
    const int stride = tokens_ref + tokens_hyp;
    const int length = min(c[0] + c[1] + c[2] + c[3], stride);     // (it is at most N + M on a table this library wrote)
    ops_length[pair] = length;
    if (statistics) atomicAdd(statistics + STATS, 1ull);
    const int* r_src = ref + (size_t)pair * tokens_ref;
    const int* h_src = hyp + (size_t)pair * tokens_hyp;
    int i = min(len_ref[pair], tokens_ref), j = min(len_hyp[pair], tokens_hyp);   // the table cell, (N, M) first
    int* out = ops + (size_t)pair * stride * 3;
    for (int at = length - 1; at >= 0 && (i > 0 || j > 0); --at) {
        uint32_t dir = i > 0 ? 1 : 2;                          // column 0: deletions only; row 0: insertions only
        if (i > 0 && j > 0) {
            const int a = i - 1, lane = (a & 255) >> 2;
            const size_t word = (((size_t)pair * blocks + (a >> 8)) * steps + j + lane) * 64 + lane;
            dir = (dirs[word] >> (8 * (a & 3))) & 3;
        }
        int kind, oi = i - 1, oj = j - 1, cell;
        if (dir == 0) {
            const int p = r_src[oi], q = h_src[oj];
            kind = p != q; cell = p * (NP + 1) + q;
            --i; --j;
        } else if (dir == 1) {
            kind = 2; cell = r_src[oi] * (NP + 1) + NP; oj = -1;
            --i;
        } else {
            kind = 3; cell = NP * (NP + 1) + h_src[oj]; oi = -1;
            --j;
        }
        out[at * 3 + 0] = kind; out[at * 3 + 1] = oi; out[at * 3 + 2] = oj;
        if (statistics) atomicAdd(statistics + cell, 1ull);
    }
}

}  // namespace

extern "C" {

size_t ppg_edit_workspace_bytes(int pairs, int tokens_ref, int tokens_hyp, int want_ops) {
    if (pairs <= 0 || pairs > PPG_EDIT_MAX_PAIRS || tokens_ref < 0 || tokens_hyp < 0 ||
        tokens_ref > PPG_EDIT_MAX_TOKENS || tokens_hyp > PPG_EDIT_MAX_TOKENS)
        return 0;
    return layout(pairs, tokens_ref, tokens_hyp, want_ops).bytes;
}

int ppg_edit_distance(int device, const int32_t* ref, int tokens_ref, const int32_t* hyp, int tokens_hyp, int pairs,
                      const int32_t* lengths_ref, const int32_t* lengths_hyp, const float* sub, const float* del,
                      const float* ins, float* total, int32_t* counts, int32_t* ops, int32_t* ops_length,
                      int64_t* statistics, void* workspace, size_t workspace_bytes, void* stream) {
    if (!lengths_ref || !lengths_hyp || !total || !counts || !workspace || pairs <= 0 || tokens_ref < 0 ||
        tokens_hyp < 0 || (!ref && tokens_ref) || (!hyp && tokens_hyp))
        return ppg::fail_message(PPG_EINVAL, "edit: bad argument");
    if (tokens_ref > PPG_EDIT_MAX_TOKENS || tokens_hyp > PPG_EDIT_MAX_TOKENS)
        return ppg::fail_message(PPG_EINVAL, "edit: %d x %d tokens, at most %d per side", tokens_ref, tokens_hyp,
                                 PPG_EDIT_MAX_TOKENS);
    if (pairs > PPG_EDIT_MAX_PAIRS)
        return ppg::fail_message(PPG_EINVAL, "edit: %d pairs, at most %d per call", pairs, PPG_EDIT_MAX_PAIRS);
    if ((sub || del || ins) && !(sub && del && ins))
        return ppg::fail_message(PPG_EINVAL, "edit: sub, del and ins are all NULL (unit costs) or all given");
    if (ops_length && !ops) return ppg::fail_message(PPG_EINVAL, "edit: ops_length needs ops");
    if (ops && !ops_length) return ppg::fail_message(PPG_EINVAL, "edit: ops needs ops_length");
    if (statistics && !ops) return ppg::fail_message(PPG_EINVAL, "edit: statistics need ops");
    const Layout w = layout(pairs, tokens_ref, tokens_hyp, ops != nullptr);
    if (workspace_bytes < w.bytes)
        return ppg::fail_message(PPG_EINVAL, "edit: workspace of %zu bytes, %zu needed", workspace_bytes, w.bytes);
    if (reinterpret_cast<uintptr_t>(workspace) % 16)
        return ppg::fail_message(PPG_EINVAL, "edit: workspace must be 16-byte aligned");
    if (hipSetDevice(device) != hipSuccess) return ppg::fail_message(PPG_EDEVICE, "no HIP device: the post-ops have no CPU path");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    int* valid = reinterpret_cast<int*>(ws + w.valid);
    uint32_t* dirs = ops ? reinterpret_cast<uint32_t*>(ws + w.dirs) : nullptr;
    const size_t lds = (size_t)(tokens_hyp + 1) * (sizeof(float) + sizeof(int));
    if (ops) {
        hipLaunchKernelGGL(edit_programme<true>, dim3(pairs), dim3(64), lds, s, ref, tokens_ref, hyp, tokens_hyp,
                           lengths_ref, lengths_hyp, sub, del, ins, w.blocks, w.steps, total, counts, valid, dirs);
        hipLaunchKernelGGL(edit_traceback, dim3((pairs + 63) / 64), dim3(64), 0, s, dirs, valid, counts, pairs, ref,
                           tokens_ref, hyp, tokens_hyp, lengths_ref, lengths_hyp, w.blocks, w.steps, ops, ops_length,
                           reinterpret_cast<unsigned long long*>(statistics));
    } else {
        hipLaunchKernelGGL(edit_programme<false>, dim3(pairs), dim3(64), lds, s, ref, tokens_ref, hyp, tokens_hyp,
                           lengths_ref, lengths_hyp, sub, del, ins, w.blocks, w.steps, total, counts, valid, dirs);
    }
    const hipError_t he = hipGetLastError();
    return he == hipSuccess ? PPG_OK : ppg::fail_message(PPG_EDEVICE, "edit: %s", hipGetErrorString(he));
}

}  // extern "C"
