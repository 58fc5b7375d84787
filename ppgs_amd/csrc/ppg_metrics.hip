// Frame metrics on the device: the per-batch work of the reference's evaluation (ppgs/evaluate/metrics.py:
// Accuracy, CategoricalAccuracy, JensenShannon, TopKAccuracy, Loss, DistanceMatrix) as ONE launch that reads
// (batch, 40, frames) logits and (batch, frames) labels once and adds into a PpgMetricsState (include/ppgs_amd.h).
//
// One thread per frame, the 40 logits in registers, loads coalesced over frames (as ppg_postops.hip).
// Every accumulator is a 64-bit integer (counts, and fp32 values rounded once to 2^-32), so addition is exact and
// the state does not depend on the order anything was added in.
//
// Accumulation: a workgroup keeps both 40 x 40 matrices and the scalars in LDS and adds its non-zero cells to the
// state with one global vector atomic each when it is done.  The matrix rows are data dependent (label, argmax)
// and neighbouring frames share them (a phoneme lasts several frames), so 64 lanes adding their own frame's row
// would meet on the same LDS addresses.  Instead a wave lays its 64 frames' probabilities down in LDS, frame-major
// with a stride of 41 words (conflict-free both ways), and turns round: lane c takes COLUMN c, walks the 64 frames,
// sums a run of equal rows in a register and adds to LDS where the row changes -- 40 lanes on 40 different
// addresses, nothing to serialise, and the number of LDS atomics follows the number of runs, not of frames.
#include "../../include/ppgs_amd.h"

#include <hip/hip_runtime.h>

namespace ppg {
int fail_message(int code, const char* fmt, ...);
}

namespace {

constexpr int NP = PPG_METRICS_CLASSES;
constexpr int WAVES = 2;
constexpr int THREADS = WAVES * 64;
constexpr int STRIDE = NP + 1;          // words between two frames of the probability tile
constexpr int MAX_BLOCKS = 256;         // grid-stride beyond: fewer workgroups, fewer flushes
constexpr int NSCALAR = 8;              // leading int64 fields of PpgMetricsState

static_assert(sizeof(PpgMetricsState) == (NSCALAR + 2 * NP + 2 * NP * NP) * 8, "PpgMetricsState layout");

typedef unsigned long long u64;

struct MetricsArgs {
    const float* logits;
    const void* labels;
    const long long* lengths;
    const float* mix;
    const float* class_weights;
    const float* loss_weights;
    u64* state;
    long long total;       // batch * frames
    int frames;
    int k;
    int label64;
};

// fp32 -> units of 2^-32, rounded once (the product is exact in double); [0, 2^20], NaN -> 0
__device__ inline u64 to_fixed(float v) {
    v = fminf(fmaxf(v, 0.f), 1048576.f);
    return (u64)__double2ll_rn((double)v * 4294967296.0);
}

__device__ inline u64 wave_sum(u64 v) {
#pragma unroll
    for (int offset = 32; offset; offset >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, offset);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), offset);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}

__device__ inline int wave_count(bool flag) { return __popcll(__ballot(flag)); }

__global__ __launch_bounds__(THREADS) void metrics_kernel(MetricsArgs a)
{
    __shared__ u64 acc[NSCALAR + 2 * NP + 2 * NP * NP];      // the workgroup's PpgMetricsState
    __shared__ float tile[WAVES][64 * STRIDE];               // softmax of the wave's frames
    __shared__ int rows[WAVES][2][64];                       // per frame: distance row, confusion row (-1: none)
    for (int i = threadIdx.x; i < NSCALAR + 2 * NP + 2 * NP * NP; i += THREADS) acc[i] = 0;
    __syncthreads();
    u64* const scalars = acc;
    u64* const class_total = acc + NSCALAR;
    u64* const class_count = class_total + NP;
    u64* const distance = class_count + NP;
    u64* const confusion = distance + NP * NP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tiles = (a.total + THREADS - 1) / THREADS;

    for (long long t0 = blockIdx.x; t0 < tiles; t0 += gridDim.x) {
        const long long f = t0 * THREADS + threadIdx.x;
        long long label = -100;
        int b = 0, t = 0;
        if (f < a.total) {
            b = (int)(f / a.frames);
            t = (int)(f - (long long)b * a.frames);
            label = a.label64 ? static_cast<const long long*>(a.labels)[f] : (long long)static_cast<const int*>(a.labels)[f];
            if (a.lengths && t >= a.lengths[b]) label = -100;
        }
        const bool counts = label != -100;
        const bool valid = counts && label >= 0 && label < NP;
        const int lab = valid ? (int)label : 0;
        bool correct = false, in_topk = false;
        u64 loss_fix = 0, weight_fix = 0, jsd_fix = 0;
        int row_distance = -1;
        if (valid) {
            const float* src = a.logits + ((size_t)b * NP) * a.frames + t;
            float x[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) x[p] = src[(size_t)p * a.frames];
            float top = x[0], own = x[0];
            int arg = 0;
#pragma unroll
            for (int p = 1; p < NP; ++p) {
                if (x[p] > top) { top = x[p]; arg = p; }          // strict: the lowest index wins a tie
                own = p == lab ? x[p] : own;
            }
            int rank = 0;                                          // logits ahead of the label's in topk order
#pragma unroll
            for (int p = 0; p < NP; ++p) rank += (x[p] > own || (x[p] == own && p < lab)) ? 1 : 0;
            correct = arg == lab;
            in_topk = rank < a.k;
            float sum = 0.f;
#pragma unroll
            for (int p = 0; p < NP; ++p) { x[p] = expf(x[p] - top); sum += x[p]; }
            float loss = logf(sum) - (own - top);                  // -log_softmax[label]
            if (a.loss_weights) {
                const float w = a.loss_weights[lab];
                loss *= w;
                weight_fix = to_fixed(w);
            }
            loss_fix = to_fixed(loss);
            float best = -1.f;
            float* dst = &tile[wave][lane * STRIDE];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                x[p] = x[p] / sum;
                dst[p] = x[p];
                const float weighted = a.class_weights ? __fmul_rn(x[p], a.class_weights[p]) : x[p];
                if (weighted > best) { best = weighted; row_distance = p; }
            }
            if (row_distance < 0) row_distance = 0;                // (non-finite logits)
            // ppg_distance against the one-hot target (ppg_postops.hip: distance_kernel)
            const float lo = 1e-8f, hi = 1.f - 1e-8f;
#pragma unroll
            for (int p = 0; p < NP; ++p) x[p] = fminf(fmaxf(x[p], lo), hi);
            float jsd = 0.f;
            if (a.mix) {
#pragma unroll 1
                for (int p = 0; p < NP; ++p) {
                    const float* m = a.mix + p * NP;               // the same address in every lane: scalar loads
                    float u = 0.f, v = 0.f;
#pragma unroll
                    for (int q = 0; q < NP; ++q) { u += m[q] * x[q]; v += m[q] * (q == lab ? hi : lo); }
                    const float lm = logf((u + v) * 0.5f);
                    const float ku = u * (logf(u) - lm), kv = v * (logf(v) - lm);
                    jsd += sqrtf(fmaxf((ku + kv) * 0.5f, 0.f));
                }
            } else {
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const float u = x[p], v = p == lab ? hi : lo;
                    const float lm = logf((u + v) * 0.5f);
                    const float ku = u * (logf(u) - lm), kv = v * (logf(v) - lm);
                    jsd += sqrtf(fmaxf((ku + kv) * 0.5f, 0.f));
                }
            }
            jsd_fix = to_fixed(jsd);
            atomicAdd(&class_count[lab], 1ull);                    // (a handful of addresses per wave)
            if (correct) atomicAdd(&class_total[lab], 1ull);
        }
        rows[wave][0][lane] = row_distance;
        rows[wave][1][lane] = valid ? lab : -1;

        const int n_count = wave_count(valid), n_correct = wave_count(correct), n_topk = wave_count(in_topk);
        const int n_invalid = wave_count(counts && !valid);
        loss_fix = wave_sum(loss_fix);
        weight_fix = wave_sum(weight_fix);
        jsd_fix = wave_sum(jsd_fix);
        if (lane == 0 && (n_count | n_invalid)) {
            atomicAdd(&scalars[0], (u64)n_count);
            atomicAdd(&scalars[1], (u64)n_correct);
            atomicAdd(&scalars[2], (u64)n_topk);
            atomicAdd(&scalars[3], (u64)n_invalid);
            atomicAdd(&scalars[4], loss_fix);
            atomicAdd(&scalars[5], weight_fix);
            atomicAdd(&scalars[6], jsd_fix);
        }
        __syncthreads();                                           // the wave's tile and rows are in LDS

        if (lane < NP && n_count) {
            const float w = a.class_weights ? a.class_weights[lane] : 1.f;
            u64 sum_d = 0, sum_c = 0;
            int cur_d = -1, cur_c = -1;
            for (int i = 0; i < 64; ++i) {
                const int rd = rows[wave][0][i], rc = rows[wave][1][i];     // the same in every lane
                if (rc < 0) continue;
                const float p = tile[wave][i * STRIDE + lane];
                if (rd != cur_d) {
                    if (sum_d) atomicAdd(&distance[cur_d * NP + lane], sum_d);
                    cur_d = rd; sum_d = 0;
                }
                if (rc != cur_c) {
                    if (sum_c) atomicAdd(&confusion[cur_c * NP + lane], sum_c);
                    cur_c = rc; sum_c = 0;
                }
                sum_d += to_fixed(a.class_weights ? __fmul_rn(p, w) : p);
                sum_c += to_fixed(p);
            }
            if (sum_d) atomicAdd(&distance[cur_d * NP + lane], sum_d);
            if (sum_c) atomicAdd(&confusion[cur_c * NP + lane], sum_c);
        }
        __syncthreads();                                           // before the next tile overwrites them
    }

    for (int i = threadIdx.x; i < NSCALAR + 2 * NP + 2 * NP * NP; i += THREADS) {
        const u64 v = acc[i];
        if (v) atomicAdd(&a.state[i], v);
    }
}

}  // namespace

extern "C" {

size_t ppg_metrics_state_bytes(void) { return sizeof(PpgMetricsState); }

int ppg_metrics_reset(int device, PpgMetricsState* state, void* stream) {
    if (!state) return ppg::fail_message(PPG_EINVAL, "metrics_reset: bad argument");
    if (hipSetDevice(device) != hipSuccess) return ppg::fail_message(PPG_EDEVICE, "no HIP device: the metrics have no CPU path");
    const hipError_t he = hipMemsetAsync(state, 0, sizeof(PpgMetricsState), static_cast<hipStream_t>(stream));
    return he == hipSuccess ? PPG_OK : ppg::fail_message(PPG_EDEVICE, "metrics_reset: %s", hipGetErrorString(he));
}

int ppg_metrics_update(int device, const float* logits, const void* labels, int label_is_int64,
                       const int64_t* lengths, int batch, int frames, int k, const float* mix,
                       const float* class_weights, const float* loss_weights, PpgMetricsState* state,
                       void* stream) {
    if (!logits || !labels || !state || batch < 0 || frames < 0)
        return ppg::fail_message(PPG_EINVAL, "metrics_update: bad argument");
    if (k < 1 || k > 8) return ppg::fail_message(PPG_EINVAL, "metrics_update: top-k needs 1 <= k <= 8");
    if (reinterpret_cast<uintptr_t>(state) % 8)
        return ppg::fail_message(PPG_EINVAL, "metrics_update: the state must be 8-byte aligned");
    if (hipSetDevice(device) != hipSuccess) return ppg::fail_message(PPG_EDEVICE, "no HIP device: the metrics have no CPU path");
    if (batch == 0 || frames == 0) return PPG_OK;
    MetricsArgs args;
    args.logits = logits;
    args.labels = labels;
    args.lengths = reinterpret_cast<const long long*>(lengths);
    args.mix = mix;
    args.class_weights = class_weights;
    args.loss_weights = loss_weights;
    args.state = reinterpret_cast<u64*>(state);
    args.total = (long long)batch * frames;
    args.frames = frames;
    args.k = k;
    args.label64 = label_is_int64 ? 1 : 0;
    const long long tiles = (args.total + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(metrics_kernel, dim3((unsigned)(tiles < MAX_BLOCKS ? tiles : MAX_BLOCKS)), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream), args);
    const hipError_t he = hipGetLastError();
    return he == hipSuccess ? PPG_OK : ppg::fail_message(PPG_EDEVICE, "metrics_update: %s", hipGetErrorString(he));
}

}  // extern "C"
