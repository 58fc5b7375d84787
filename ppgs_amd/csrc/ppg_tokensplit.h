// What the token-split kernels -- the generic linear / conv kernel (ppg_linear.h) and the fused FFN (ppg_ffn.h) --
// share: the LayerNorm epilogues and the staging of their parameters.  Each family is compiled once per precision
// (ppg_linear_<precision>.hip, ppg_ffn_<precision>.hip), so that a clean build is as parallel as it has units.
// See ppg_device.h for the operand orientation shared by all of them.
#pragma once

#include "ppg_device.h"
#include "ppg_launch.h"

#include <stdlib.h>
#include <string.h>
#include "ppg_lds.h"

#include <limits.h>
#include <type_traits>

namespace {

constexpr float kLnEps = 1e-5f;

// ---------------------------------------------------------------------------
// acc <- LayerNorm(acc + bias + X[m][:]), acc in the transposed C layout
// (lane: token = tok0 + 16t + idx, features pair_feature(nb, g) + r).
// MODE LN_EPILOGUE: result to X (fp32) and Xb (bf16 copy, bf16 mode).
// MODE LN_KEEP: result stays in acc, nothing is stored (the fused FFN's LN1:
//   x1 is both the next GEMM's operand and, left in the accumulators that the
//   FFN then adds to, the second residual).
// MODE LN_NO_RESIDUAL: acc already contains the residual; stores like LN_EPILOGUE.
// MODE LN_NO_RESIDUAL_KEEP: same input, result to X only and kept in acc (the
//   next layer's Q/K/V projection follows in the same kernel, no bf16 copy needed).
// lnp = [bias | gamma | beta], H floats each, in LDS: read from global per
// (feature block, token block) these were 60 % of the epilogue's memory
// instructions, all queueing behind the residual loads and the stores in the
// CU's one address unit.  Loops run feature-block-outer so each parameter
// vector is fetched once for all NT token blocks.
// ---------------------------------------------------------------------------
enum { LN_EPILOGUE = 0, LN_KEEP = 1, LN_NO_RESIDUAL = 2, LN_NO_RESIDUAL_KEEP = 3 };
template <class P, int NB, int NT, int MODE>
__device__ __forceinline__ void resln(
    f32x4 (&acc)[NB][NT], const float* lnp, float* X, char* Xb, int H,
    int tok0, int M, int idx, int g)
{
    bool ok[NT];
    float* xrow[NT];
    float sum[NT], mean[NT], rstd[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int m = tok0 + 16 * t + idx;
        ok[t] = m < M;
        xrow[t] = X + (size_t)(ok[t] ? m : 0) * H;
        sum[t] = 0.f;
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int n = pair_feature(nb, g);
        const float4 bv = *reinterpret_cast<const float4*>(lnp + n);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (MODE != LN_NO_RESIDUAL && MODE != LN_NO_RESIDUAL_KEEP) {
                if (ok[t]) rv = *reinterpret_cast<const float4*>(xrow[t] + n);
            }
            acc[nb][t][0] += bv.x + rv.x;
            acc[nb][t][1] += bv.y + rv.y;
            acc[nb][t][2] += bv.z + rv.z;
            acc[nb][t][3] += bv.w + rv.w;
            sum[t] += (acc[nb][t][0] + acc[nb][t][1]) + (acc[nb][t][2] + acc[nb][t][3]);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        mean[t] = wave_sum_g(sum[t]) / (float)H;
        float sq = 0.f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float d = acc[nb][t][r] - mean[t];
                sq += d * d;
            }
        }
        const float var = wave_sum_g(sq) / (float)H;
        rstd[t] = 1.0f / sqrtf(var + kLnEps);
    }
    PairStore<P> pair[NT];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int n = pair_feature(nb, g);
        const float4 gv = *reinterpret_cast<const float4*>(lnp + H + n);
        const float4 ev = *reinterpret_cast<const float4*>(lnp + 2 * H + n);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float y0 = (acc[nb][t][0] - mean[t]) * rstd[t] * gv.x + ev.x;
            const float y1 = (acc[nb][t][1] - mean[t]) * rstd[t] * gv.y + ev.y;
            const float y2 = (acc[nb][t][2] - mean[t]) * rstd[t] * gv.z + ev.z;
            const float y3 = (acc[nb][t][3] - mean[t]) * rstd[t] * gv.w + ev.w;
            if constexpr (MODE == LN_KEEP || MODE == LN_NO_RESIDUAL_KEEP) acc[nb][t] = f32x4{y0, y1, y2, y3};
            if constexpr (MODE != LN_KEEP) {
                if (ok[t]) {
                    *reinterpret_cast<float4*>(xrow[t] + n) = make_float4(y0, y1, y2, y3);
                    if constexpr ((P::kIsBF16 || P::kSplit) && MODE != LN_NO_RESIDUAL_KEEP)
                        pair[t].put(Xb + (size_t)(tok0 + 16 * t + idx) * H * P::kBytes + P::row_byte(n & ~7), nb & 1, y0, y1, y2, y3);
                }
            }
        }
    }
}

// Cooperative copy of `count` float vectors of H floats each (global, given
// as pointers) into consecutive LDS rows; the caller synchronises.
// (`used`: the compiler narrows the arguments of a unit-local function to what the unit's callers pass BEFORE it
// inlines it, so a caller's code depended on which other kernels shared its unit -- the hidden-512 FFN kernels, H a
// constant, came out a few instructions different once the linear kernels, H from the arguments, had left their unit.
// A function marked `used` is not narrowed: every caller gets the code it got beside a caller with an unknown H.)
__attribute__((used)) __device__ __forceinline__ void stage_params(float* lds, int H, int tid, const float* p0, const float* p1, const float* p2) {
    for (int i = tid; i < 3 * H / 4; i += 256) {
        const int v = i / (H / 4), j = i - v * (H / 4);
        const float* src = v == 0 ? p0 : (v == 1 ? p1 : p2);
        reinterpret_cast<float4*>(lds)[i] = reinterpret_cast<const float4*>(src)[j];
    }
}

// The fused FFN's LN1: acc <- LayerNorm(acc + bias + X[m][:]) in registers,
// nothing stored, plus the result packed as the next GEMM's B fragments xf
// (paired feature blocks 2p, 2p+1 = K-group p; fp32: block nb = K-group nb in
// the column order W1 was uploaded in).  The accumulators are MFMA results in
// AGPRs and must be back there for the chunk loop, whose register budget has
// no slack: one 16-token block at a time moves to VGPRs for the LayerNorm
// arithmetic, and the asm pins on the accumulators on either side keep the
// allocator from blending this code's live ranges with the GEMMs' around it
// (unpinned, it spills most of the accumulators to scratch while they are
// being computed and the chunk loop runs 15 % slower; pinning xf as well costs
// 12 % -- measured, PPG_FFN_TIMING).
// Residual row of the wave's token block t (lane: token idx, features of lane group g)
template <int NB>
__device__ __forceinline__ void load_residual_rows(float4 (&rv)[NB], const float* X, int H, int m, int M, int g) {
    const float* xrow = X + (size_t)(m < M ? m : 0) * H;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        rv[nb] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < M) rv[nb] = *reinterpret_cast<const float4*>(xrow + pair_feature(nb, g));
    }
}

template <class P, int NB, int NT, int XG, int NTX>
__device__ __forceinline__ void ln_keep(
    f32x4 (&acc)[NB][NT], u32x4 (&xf)[XG][NTX], const float* lnp, const float* X, int H,
    int tok0, int M, int idx, int g, float4 (&rcur)[NB] /* rows of block 0, loaded by the caller */)
{
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int t = 0; t < NT; ++t) asm volatile("" : "+a"(acc[nb][t]));
    // residual rows: block t+1 is loaded while block t is normalised
    auto load_rows = [&](int t, float4 (&rv)[NB]) { load_residual_rows<NB>(rv, X, H, tok0 + 16 * t + idx, M, g); };
    float4 rnext[NB];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t + 1 < NT) load_rows(t + 1, rnext);
        f32x4 v[NB];
        float sum = 0.f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int n = pair_feature(nb, g);
            const float4 bv = *reinterpret_cast<const float4*>(lnp + n);
            const float4 rv = rcur[nb];
            v[nb] = acc[nb][t] + f32x4{bv.x + rv.x, bv.y + rv.y, bv.z + rv.z, bv.w + rv.w};
            sum += (v[nb][0] + v[nb][1]) + (v[nb][2] + v[nb][3]);
        }
        const float mean = wave_sum_g(sum) / (float)H;
        float sq = 0.f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float d = v[nb][r] - mean;
                sq += d * d;
            }
        }
        const float rstd = 1.0f / sqrtf(wave_sum_g(sq) / (float)H + kLnEps);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int n = pair_feature(nb, g);
            const float4 gv = *reinterpret_cast<const float4*>(lnp + H + n);
            const float4 ev = *reinterpret_cast<const float4*>(lnp + 2 * H + n);
            v[nb][0] = (v[nb][0] - mean) * rstd * gv.x + ev.x;
            v[nb][1] = (v[nb][1] - mean) * rstd * gv.y + ev.y;
            v[nb][2] = (v[nb][2] - mean) * rstd * gv.z + ev.z;
            v[nb][3] = (v[nb][3] - mean) * rstd * gv.w + ev.w;
        }
#pragma unroll
        for (int kg = 0; kg < XG; ++kg) {
            if constexpr (P::kIsBF16) {
                xf[kg][t] = u32x4{P::pack2(v[2 * kg][0], v[2 * kg][1]), P::pack2(v[2 * kg][2], v[2 * kg][3]),
                                  P::pack2(v[2 * kg + 1][0], v[2 * kg + 1][1]), P::pack2(v[2 * kg + 1][2], v[2 * kg + 1][3])};
            } else {
                xf[kg][t] = u32x4{__float_as_uint(v[kg][0]), __float_as_uint(v[kg][1]), __float_as_uint(v[kg][2]), __float_as_uint(v[kg][3])};
            }
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            acc[nb][t] = v[nb];
            asm volatile("" : "+a"(acc[nb][t]));
        }
        if (t + 1 < NT) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) rcur[nb] = rnext[nb];
        }
    }
}

}  // namespace
