// Pronunciation distance and alignment for PPGs of different lengths: dynamic time warping over the per-frame term
// of ppg_distance (ppg_postops.hip), on the device.
//
//   C[i, j] = sum_p sqrt(max(0, (KL(x'_i || m) + KL(y'_j || m)) / 2)),  m = (x'_i + y'_j) / 2,  x' = clamp + mix
//   D[0, 0] = C[0, 0];  D[i, j] = C[i, j] + min(D[i-1, j-1], D[i-1, j], D[i, j-1])       (fp32, missing = +inf)
//   ties: the diagonal first, then (i-1, j), then (i, j-1); the minimum is comparisons only.
//
// Four kernels on one stream, no allocation, no synchronisation:
//   dtw_prepare    one thread per frame of either side (ONE piece of code for both, so equal frames give equal
//                  bits): clamp, mix, and (a, log a) per phoneme, written frame-major.
//   dtw_cost       one workgroup per 64 rows x 64 steps of the SKEWED cost image the dynamic programme streams:
//                  rows come in blocks of 256 = 64 lanes x 4 rows; lane l of a block meets column s - l at step s;
//                  the image holds, per block and step, 64 lanes x 4 costs = 1 KiB, so the programme's read is one
//                  16-byte load per lane and step and the cost kernel's write is 256 B per wave and step.
//   dtw_programme  one wave per pair.  Each lane keeps its 4 rows of the previous column in registers, takes the row
//                  above its strip from lane l - 1 by a cross-lane move, and carries the step count K beside the
//                  cost, so the distance needs neither directions nor a trace-back.  A block's last row reaches
//                  the next block through LDS.  With a path wanted it also stores one direction byte per cell.
//   dtw_traceback  one thread per pair; K is known from the programme, so the path is written in forward order.
#include "../../include/ppgs_amd.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace ppg {
int fail_message(int code, const char* fmt, ...);
}

namespace {

constexpr int NP = 40;            // phonemes
constexpr int PREP = 2 * NP;      // floats per prepared frame: (a, log a) per phoneme
constexpr int STRIP = 4;          // rows per lane
constexpr int BLOCK_ROWS = 64 * STRIP;
constexpr int YPAD = PREP + 2;    // LDS row stride of a prepared Y frame: 41 eight-byte words, odd -> no bank conflicts
constexpr int TILE_COLS = 64 + 15;   // columns a 16-lane x 64-step tile of the skewed image touches
constexpr int CHUNK = 8;          // steps per prefetch group of the programme

struct Layout {
    size_t prep_x, prep_y, cost, dirs, bytes;   // byte offsets into the workspace; dirs == 0: none
    int blocks, steps;                          // row blocks per pair, steps per block in the image (multiple of 64)
};

inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

inline Layout layout(int pairs, int frames_x, int frames_y, int want_path) {
    Layout w{};
    w.blocks = (frames_x + BLOCK_ROWS - 1) / BLOCK_ROWS;
    w.steps = (frames_y + 63 + 63) / 64 * 64;
    const size_t cells = (size_t)pairs * w.blocks * w.steps * 64;       // lanes x steps x blocks
    size_t at = 0;
    w.prep_x = at; at = align256(at + (size_t)pairs * frames_x * PREP * sizeof(float));
    w.prep_y = at; at = align256(at + (size_t)pairs * frames_y * PREP * sizeof(float));
    w.cost = at;   at = align256(at + cells * STRIP * sizeof(float));
    if (want_path) { w.dirs = at; at = align256(at + cells * sizeof(uint32_t)); }
    w.bytes = at;
    return w;
}

// side 0 = X, 1 = Y (blockIdx.z); src (pairs, 40, frames) fp32, only frames < lengths[pair] are read
__global__ __launch_bounds__(64) void dtw_prepare(const float* __restrict__ x, const float* __restrict__ y,
                                                   int frames_x, int frames_y, const int* __restrict__ len_x,
                                                   const int* __restrict__ len_y, const float* __restrict__ mix,
                                                   float* __restrict__ prep_x, float* __restrict__ prep_y)
{
    __shared__ float m[NP * NP];
    if (mix) for (int i = threadIdx.x; i < NP * NP; i += 64) m[i] = mix[i];
    __syncthreads();
    const int side = blockIdx.z, pair = blockIdx.y;
    const int frames = side ? frames_y : frames_x;
    const int length = side ? len_y[pair] : len_x[pair];       // (t < frames bounds it)
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= frames || t >= length) return;
    const float* src = (side ? y : x) + (size_t)pair * NP * frames + t;
    float* dst = (side ? prep_y : prep_x) + ((size_t)pair * frames + t) * PREP;
    float v[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) v[p] = fminf(fmaxf(src[(size_t)p * frames], 1e-8f), 1.f - 1e-8f);
#pragma unroll 1
    for (int p = 0; p < NP; ++p) {
        float a = 0.f;
        if (mix) {
#pragma unroll
            for (int q = 0; q < NP; ++q) a += m[p * NP + q] * v[q];
        } else {
#pragma unroll
            for (int q = 0; q < NP; ++q) a = q == p ? v[q] : a;
        }
        *reinterpret_cast<float2*>(dst + 2 * p) = make_float2(a, logf(a));
    }
}

// grid (steps / 64, blocks * 4, pairs), 256 threads: thread = (row r of the tile's 64, wave w of 4); wave w does
// steps w * 16 .. + 15 of the tile's 64.  The thread's X frame sits in registers, the 79 Y frames in LDS.
__global__ __launch_bounds__(256) void dtw_cost(const float* __restrict__ prep_x, const float* __restrict__ prep_y,
                                                 int frames_x, int frames_y, const int* __restrict__ len_x,
                                                 const int* __restrict__ len_y, int blocks, int steps,
                                                 float* __restrict__ cost)
{
    __shared__ float sy[TILE_COLS * YPAD];
    const int pair = blockIdx.z, block = blockIdx.y >> 2, group = blockIdx.y & 3;
    const int tx = min(len_x[pair], frames_x), ty = min(len_y[pair], frames_y);
    const int i0 = block * BLOCK_ROWS + group * 64, s0 = blockIdx.x * 64, lane0 = group * 16;
    if (i0 >= tx || s0 - (lane0 + 15) >= ty) return;         // no valid cell in this tile (uniform)
    const int jlo = s0 - (lane0 + 15);
    const float* ysrc = prep_y + (size_t)pair * frames_y * PREP;
    for (int idx = threadIdx.x; idx < TILE_COLS * PREP; idx += 256) {
        const int c = idx / PREP, e = idx - c * PREP, j = jlo + c;
        sy[c * YPAD + e] = (j >= 0 && j < ty) ? ysrc[(size_t)j * PREP + e] : 1.f;
    }
    __syncthreads();
    const int r = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = i0 + r, lane = r >> 2;
    float xa[NP], xl[NP];
    if (i < tx) {
        const float2* xsrc = reinterpret_cast<const float2*>(prep_x + ((size_t)pair * frames_x + i) * PREP);
#pragma unroll
        for (int p = 0; p < NP; ++p) { const float2 v = xsrc[p]; xa[p] = v.x; xl[p] = v.y; }
    } else {
#pragma unroll
        for (int p = 0; p < NP; ++p) { xa[p] = 1.f; xl[p] = 0.f; }
    }
    float* out = cost + (((size_t)pair * blocks + block) * steps + s0) * BLOCK_ROWS + group * 64 + r;
#pragma unroll 1
    for (int u = 0; u < 16; ++u) {
        const int ds = w * 16 + u;
        const int c = ds - lane + 15;                         // 0 .. 78
        const int j = jlo + c;
        float jsd = 0.f;
        if (i < tx && j >= 0 && j < ty) {
            const float2* yc = reinterpret_cast<const float2*>(sy + c * YPAD);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const float2 yv = yc[p];
                const float a = xa[p], b = yv.x;
                const float la = logf((a + b) * 0.5f);
                const float kx = a * (xl[p] - la), ky = b * (yv.y - la);
                const float avg = fmaxf((kx + ky) * 0.5f, 0.f);
                jsd += sqrtf(avg);
            }
        }
        out[(size_t)ds * BLOCK_ROWS] = jsd;                   // cells outside the pair hold 0, never +-inf or NaN
    }
}

// lane l <- lane l - 1; lane 0 <- first
__device__ __forceinline__ int lane_up(int v, int first) {
#ifdef PPG_DTW_BPERMUTE
    const int got = __shfl_up(v, 1, 64);
    return (threadIdx.x & 63) == 0 ? first : got;
#else
    return __builtin_amdgcn_update_dpp(first, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
#endif
}
__device__ __forceinline__ float lane_up(float v, float first) {
    return __int_as_float(lane_up(__float_as_int(v), __float_as_int(first)));
}

// one cell: best predecessor of (diagonal, up, left) in that order of preference, comparisons only
__device__ __forceinline__ void relax(float c, float dd, int dn, float ud, int un, float& d, int& n, uint32_t& dir) {
    float best = dd; int steps = dn; dir = 0;
    if (ud < best) { best = ud; steps = un; dir = 1; }
    if (d < best) { best = d; steps = n; dir = 2; }
    d = c + best;
    n = steps + 1;
}

// grid (pairs), 64 threads; dynamic LDS: frames_y x (float + int), the last row of the previous block
template <bool kPath>
__global__ __launch_bounds__(64) void dtw_programme(const float* __restrict__ cost, int frames_x, int frames_y,
                                                     const int* __restrict__ len_x, const int* __restrict__ len_y,
                                                     int blocks, int steps, float* __restrict__ total,
                                                     int* __restrict__ count, uint32_t* __restrict__ dirs)
{
    extern __shared__ float edge[];
    float* edge_d = edge;
    int* edge_n = reinterpret_cast<int*>(edge + frames_y);
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int tx = min(len_x[pair], frames_x), ty = min(len_y[pair], frames_y);
    const float inf = INFINITY;
    if (tx <= 0 || ty <= 0) {                                  // not a pair: the caller's lengths are wrong
        if (lane == 0) { total[pair] = NAN; count[pair] = 0; }
        return;
    }
    const int used = (tx + BLOCK_ROWS - 1) / BLOCK_ROWS;
    float d[STRIP]; int n[STRIP];
    for (int block = 0; block < used; ++block) {
        const int rows = min(tx - block * BLOCK_ROWS, BLOCK_ROWS);
        const int lanes = (rows + STRIP - 1) / STRIP;
        const int nsteps = ty + lanes - 1;
        const bool hand_on = block + 1 < used;                 // then rows == BLOCK_ROWS and lane 63 holds the last row
        const size_t base = ((size_t)pair * blocks + block) * steps;
        const float4* src = reinterpret_cast<const float4*>(cost) + base * 64 + lane;
        uint32_t* dst = kPath ? dirs + base * 64 + lane : nullptr;
#pragma unroll
        for (int k = 0; k < STRIP; ++k) { d[k] = inf; n[k] = 0; }
        // the cell above-left of the strip's column: the virtual origin D[-1, -1] = 0 for the very first cell
        float diag_d = (block == 0 && lane == 0) ? 0.f : inf;
        int diag_n = 0;
        float top_d = inf; int top_n = 0;                      // this chunk of the previous block's last row, one column per lane
        float4 next[CHUNK];
#pragma unroll
        for (int u = 0; u < CHUNK; ++u) next[u] = src[(size_t)min(u, steps - 1) * 64];
        for (int s0 = 0; s0 < nsteps; s0 += CHUNK) {
            float4 cur[CHUNK];
#pragma unroll
            for (int u = 0; u < CHUNK; ++u) cur[u] = next[u];
#pragma unroll
            for (int u = 0; u < CHUNK; ++u) next[u] = src[(size_t)min(s0 + CHUNK + u, steps - 1) * 64];
            if (block > 0 && (s0 & 63) == 0) {
                const int col = s0 + lane;
                top_d = col < ty ? edge_d[col] : inf;
                top_n = col < ty ? edge_n[col] : 0;
            }
#pragma unroll
            for (int u = 0; u < CHUNK; ++u) {
                const int s = s0 + u;
                const float first_d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(top_d), s & 63));
                const int first_n = __builtin_amdgcn_readlane(top_n, s & 63);
                const float up_d = lane_up(d[STRIP - 1], first_d);
                const int up_n = lane_up(n[STRIP - 1], first_n);
                const int j = s - lane;
                if (j >= 0 && j < ty && lane < lanes) {
                    const float c[STRIP] = {cur[u].x, cur[u].y, cur[u].z, cur[u].w};
                    float pd = diag_d, qd = up_d; int pn = diag_n, qn = up_n;     // diagonal and upper neighbour of row k
                    uint32_t code = 0;
#pragma unroll
                    for (int k = 0; k < STRIP; ++k) {
                        const float old_d = d[k]; const int old_n = n[k];
                        uint32_t dir;
                        relax(c[k], pd, pn, qd, qn, d[k], n[k], dir);
                        code |= dir << (8 * k);
                        pd = old_d; pn = old_n; qd = d[k]; qn = n[k];
                    }
                    if (kPath) dst[(size_t)s * 64] = code;
                    if (hand_on && lane == 63) { edge_d[j] = d[STRIP - 1]; edge_n[j] = n[STRIP - 1]; }
                }
                if (j >= -1) { diag_d = up_d; diag_n = up_n; }
            }
        }
    }
    const int last = tx - 1 - (used - 1) * BLOCK_ROWS;         // row of the final cell inside the last block
    if (lane == last / STRIP) {
        const int k = last % STRIP;
        float rd = d[0]; int rn = n[0];
#pragma unroll
        for (int q = 1; q < STRIP; ++q) { rd = k == q ? d[q] : rd; rn = k == q ? n[q] : rn; }
        total[pair] = rd;
        count[pair] = rn;
    }
}

// grid (ceil(pairs / 64)), 64 threads: thread = pair
__global__ __launch_bounds__(64) void dtw_traceback(const uint32_t* __restrict__ dirs, const float* __restrict__ cost,
                                                     int pairs, int frames_x, int frames_y,
                                                     const int* __restrict__ len_x,
                                                     const int* __restrict__ len_y, int blocks, int steps,
                                                     const int* __restrict__ count, int path_stride,
                                                     int* __restrict__ path, int* __restrict__ path_length,
                                                     float* __restrict__ path_cost)
{
    const int pair = blockIdx.x * 64 + threadIdx.x;
    if (pair >= pairs) return;
    const int total = count[pair];
    path_length[pair] = total;
    int i = min(len_x[pair], frames_x) - 1, j = min(len_y[pair], frames_y) - 1;
    int2* out = reinterpret_cast<int2*>(path) + (size_t)pair * path_stride;
    float* out_cost = path_cost ? path_cost + (size_t)pair * path_stride : nullptr;
    for (int at = min(total, path_stride) - 1; at >= 0; --at) {
        const size_t word = (((size_t)pair * blocks + (i >> 8)) * steps + j + ((i & 255) >> 2)) * 64 + ((i & 255) >> 2);
        out[at] = make_int2(i, j);
        if (out_cost) out_cost[at] = cost[word * STRIP + (i & 3)];
        if (i == 0 && j == 0) break;
        const uint32_t dir = (dirs[word] >> (8 * (i & 3))) & 3;
        i -= dir != 2;
        j -= dir != 1;
        if (i < 0 || j < 0) break;                             // cannot happen on a table this library wrote
    }
}

}  // namespace

extern "C" {

size_t ppg_dtw_workspace_bytes(int pairs, int frames_x, int frames_y, int want_path) {
    if (pairs <= 0 || pairs > PPG_DTW_MAX_PAIRS || frames_x <= 0 || frames_y <= 0 ||
        frames_x > PPG_DTW_MAX_FRAMES || frames_y > PPG_DTW_MAX_FRAMES)
        return 0;
    return layout(pairs, frames_x, frames_y, want_path).bytes;
}

int ppg_dtw(int device, const float* ppg_x, int frames_x, const float* ppg_y, int frames_y, int pairs,
            const int32_t* lengths_x, const int32_t* lengths_y, const float* mix, float* total, int32_t* steps,
            int32_t* path, int32_t* path_length, float* path_cost, void* workspace, size_t workspace_bytes,
            void* stream) {
    if (!ppg_x || !ppg_y || !lengths_x || !lengths_y || !total || !steps || !workspace || pairs <= 0 ||
        frames_x <= 0 || frames_y <= 0)
        return ppg::fail_message(PPG_EINVAL, "dtw: bad argument");
    if (frames_x > PPG_DTW_MAX_FRAMES || frames_y > PPG_DTW_MAX_FRAMES)
        return ppg::fail_message(PPG_EINVAL, "dtw: %d x %d frames, at most %d per side", frames_x, frames_y,
                                 PPG_DTW_MAX_FRAMES);
    if (pairs > PPG_DTW_MAX_PAIRS)
        return ppg::fail_message(PPG_EINVAL, "dtw: %d pairs, at most %d per call", pairs, PPG_DTW_MAX_PAIRS);
    if ((path_length || path_cost) && !path)
        return ppg::fail_message(PPG_EINVAL, "dtw: path_length and path_cost need path");
    if (path && !path_length) return ppg::fail_message(PPG_EINVAL, "dtw: path needs path_length");
    const Layout w = layout(pairs, frames_x, frames_y, path != nullptr);
    if (workspace_bytes < w.bytes)
        return ppg::fail_message(PPG_EINVAL, "dtw: workspace of %zu bytes, %zu needed", workspace_bytes, w.bytes);
    if (reinterpret_cast<uintptr_t>(workspace) % 16)
        return ppg::fail_message(PPG_EINVAL, "dtw: workspace must be 16-byte aligned");
    if (hipSetDevice(device) != hipSuccess) return ppg::fail_message(PPG_EDEVICE, "no HIP device: the post-ops have no CPU path");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    float* prep_x = reinterpret_cast<float*>(ws + w.prep_x);
    float* prep_y = reinterpret_cast<float*>(ws + w.prep_y);
    float* cost = reinterpret_cast<float*>(ws + w.cost);
    uint32_t* dirs = path ? reinterpret_cast<uint32_t*>(ws + w.dirs) : nullptr;
    const int longest = frames_x > frames_y ? frames_x : frames_y;
    hipLaunchKernelGGL(dtw_prepare, dim3((longest + 63) / 64, pairs, 2), dim3(64), 0, s, ppg_x, ppg_y, frames_x,
                       frames_y, lengths_x, lengths_y, mix, prep_x, prep_y);
    hipLaunchKernelGGL(dtw_cost, dim3(w.steps / 64, w.blocks * 4, pairs), dim3(256), 0, s, prep_x, prep_y, frames_x,
                       frames_y, lengths_x, lengths_y, w.blocks, w.steps, cost);
    const size_t lds = (size_t)frames_y * (sizeof(float) + sizeof(int));
    if (path) {
        hipLaunchKernelGGL(dtw_programme<true>, dim3(pairs), dim3(64), lds, s, cost, frames_x, frames_y, lengths_x, lengths_y,
                           w.blocks, w.steps, total, steps, dirs);
        hipLaunchKernelGGL(dtw_traceback, dim3((pairs + 63) / 64), dim3(64), 0, s, dirs, cost, pairs, frames_x, frames_y,
                           lengths_x, lengths_y, w.blocks, w.steps, steps, frames_x + frames_y - 1, path, path_length, path_cost);
    } else {
        hipLaunchKernelGGL(dtw_programme<false>, dim3(pairs), dim3(64), lds, s, cost, frames_x, frames_y, lengths_x, lengths_y,
                           w.blocks, w.steps, total, steps, dirs);
    }
    const hipError_t he = hipGetLastError();
    return he == hipSuccess ? PPG_OK : ppg::fail_message(PPG_EDEVICE, "dtw: %s", hipGetErrorString(he));
}

}  // extern "C"
