// gfx950 kernels of the PPG encoder: the window gather and the fill.
// See ppg_device.h for the operand orientation.
#include "ppg_device.h"
#include "ppg_launch.h"

namespace {

// ---------------------------------------------------------------------------
// Window gather: (B, C, T) features -> token-major Xw[M][Cp] in P::elem.
// Applies the left replicate padding of chunked windows (reference
// transformer.py:54) and zero-fills padded channels / padded token rows.
// Tile = 32 channels x 64 tokens through LDS so both sides are coalesced.
// ---------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(256) void gather_kernel(GatherArgs a) {
    if (blockIdx.y == gridDim.y - 1) {
        // Housekeeping row: zero what no kernel writes but the attention tiles read
        // (masked, p = 0 -- but 0 x NaN would poison the sum): the odd 16-column
        // tail of windows whose padded length is not a multiple of 32, the slack
        // behind the last V^T column, and the q|k rows behind the last token.
        constexpr int kBytes = P::kBytes;
        for (int job = blockIdx.x; job <= a.nwin + 1; job += gridDim.x) {
            if (job == a.nwin + 1) {
                for (int i = threadIdx.x; i < a.qk_slack_bytes / 16; i += 256)
                    reinterpret_cast<uint4*>(a.qk_slack)[i] = make_uint4(0u, 0u, 0u, 0u);
                continue;
            }
            int col, count;
            if (job < a.nwin) {
                const PpgWindow w = a.win[job];
                // a window with an odd number of 16-token blocks: its last 32-column group is only half
                // written by the projections -- in the 16-bit modes the columns are permuted inside the
                // group (position 8g + 4e + r), so the unwritten ones are NOT the linear tail: clear the
                // whole group (this launch runs before the projections fill in their half)
                const int r16 = (w.frames + 15) & ~15, r32 = (w.frames + 31) & ~31;
                col = w.vt_off + r32 - 32;
                count = r32 != r16 ? 32 : 0;
            } else {
                col = a.vt_tokens;
                count = a.vt_ld - a.vt_tokens;
            }
            const int chunks = count * kBytes / 16;      // 16-column steps: whole 16-byte pieces
            for (int i = threadIdx.x; i < a.vt_rows * chunks; i += 256) {
                const int r = i / chunks, c = i - r * chunks;
                *reinterpret_cast<uint4*>(a.vt + ((size_t)r * a.vt_ld + col) * kBytes + c * 16) = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        return;
    }
    __shared__ float tile[32][65];
    const int tok0 = blockIdx.x * 64;
    const int c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 63;   // token within tile (read phase)
    const int ty = threadIdx.x >> 6;   // 0..3
    // token row of tile position tl (row map: every 16-row block of the tile has its own place)
    auto row_of = [&](int tl) { return a.rowmap ? a.rowmap[blockIdx.x * 4 + (tl >> 4)] + (tl & 15) : tok0 + tl; };
    {
        const int m = row_of(tx);
        const TokMeta tm = tok_meta(a.blk_win, a.win, m, a.M);
        int frame = -1;
        size_t base = 0;
        if (tm.w >= 0 && tm.tt < tm.frames) {
            const PpgWindow w = a.win[tm.w];
            frame = w.chunked ? max(w.start + tm.tt - a.overlap, 0) : tm.tt;
            base = (size_t)w.item * a.C * a.T;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = c0 + ty * 8 + i;
            float v = 0.f;
            if (frame >= 0 && c < a.C) {
                const size_t off = base + (size_t)c * a.T + frame;
                v = (a.dtype == PPG_DTYPE_F16)
                        ? __half2float(reinterpret_cast<const __half*>(a.feats)[off])
                        : reinterpret_cast<const float*>(a.feats)[off];
            }
            tile[ty * 8 + i][tx] = v;
        }
    }
    __syncthreads();
    {
        const int c = threadIdx.x & 31;     // channel within tile (write phase)
        const int tq = threadIdx.x >> 5;    // 0..7
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int tl = tq * 8 + i;
            const int m = row_of(tl);
            if (m < a.M && c0 + c < a.Cp) {
                const float v = tile[c][tl];
                if constexpr (P::kSplit) {
                    char* row = a.xw + (size_t)m * a.Cp * P::kBytes + P::row_byte(c0 + c);
                    uint32_t hi, lo;
                    P::split2(v, 0.f, hi, lo);
                    *reinterpret_cast<uint16_t*>(row) = (uint16_t)hi;
                    *reinterpret_cast<uint16_t*>(row + 64) = (uint16_t)lo;
                } else {
                    typename P::elem* dst = reinterpret_cast<typename P::elem*>(a.xw) + (size_t)m * a.Cp + c0 + c;
                    *dst = P::cvt1(v);
                }
            }
        }
    }
}

__global__ void fill_kernel(float* p, size_t n, float v) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}

}  // namespace

namespace ppg {

hipError_t launch_gather(int precision, const GatherArgs& a, hipStream_t s) {
    dim3 grid(a.rowmap ? (a.map_blocks + 3) / 4 : (a.M + 63) / 64, (a.Cp + 31) / 32 + 1);       // + the housekeeping row
    if (precision == PPG_PRECISION_BF16) hipLaunchKernelGGL(gather_kernel<PrecBF16>, grid, dim3(256), 0, s, a);
#if PPG_X2
    else if (precision == PPG_PRECISION_FP16X2) hipLaunchKernelGGL(gather_kernel<PrecX2>, grid, dim3(256), 0, s, a);
#endif
#if PPG_OTHER_PRECISIONS
    else if (precision == PPG_PRECISION_FP16) hipLaunchKernelGGL(gather_kernel<PrecF16>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(gather_kernel<PrecF32>, grid, dim3(256), 0, s, a);
#else
    else return hipErrorInvalidValue;
#endif
    return hipGetLastError();
}

hipError_t launch_fill(float* p, size_t n, float v, hipStream_t s) {
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(fill_kernel, dim3(blocks), dim3(256), 0, s, p, n, v);
    return hipGetLastError();
}

}  // namespace ppg
