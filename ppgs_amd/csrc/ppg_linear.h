// The generic "weights-from-LDS" linear / conv kernel with its fused epilogues, and the launchers that pick an
// instantiation.  Included by ppg_linear_<precision>.hip, which instantiate ppg::launch_linear_p for one precision
// each; ppg_linear.hip dispatches on the precision.
#pragma once

#include "ppg_tokensplit.h"

namespace {

// ---------------------------------------------------------------------------
// Generic linear / k-tap conv:  out^T[n][tok] = sum_k W[n][k] act[tok][k].
// Workgroup = 4 waves; wave owns 16*NT tokens, all NB*16 features of this
// blockIdx.y pass.  W tiles [NB*16 rows][128 B = 2 K-groups] are staged
// global -> registers -> LDS (double buffered, one barrier per tile, loads
// of tile s+1 issued before the MFMAs of tile s).
// ---------------------------------------------------------------------------
// NT <= 2 (and the 16-feature-block passes): capped at 256 registers so two
// workgroups share a CU and cover each other's LDS / barrier / issue stalls.
template <class P, int NT, int NB, int EPI>
__global__ __launch_bounds__(256, (NT <= 2 && NB <= 16) ? 2 : 1) void linear_kernel(LinearArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TILE_BYTES = NB * 16 * 128;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int idx = lane & 15;
    const int g = lane >> 4;
    const int tok0 = a.rowmap ? __builtin_amdgcn_readfirstlane(a.rowmap[blockIdx.x * 4 + wave]) : (blockIdx.x * 4 + wave) * 16 * NT;
    const int n0 = blockIdx.y * NB * 16;
    const bool swap = (EPI == EPI_QKV) && (n0 >= a.v_start);

#ifdef PPG_LIN_TIMING
    auto stamp = [&](int k) {
        if (a.dbg && tid == 0 && k < 15)
            a.dbg[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 + k] = __builtin_amdgcn_s_memtime();
    };
#else
    auto stamp = [&](int) {};
#endif
    stamp(0);
    // Window lookups (two dependent global loads) only where window positions
    // matter: the k-tap convs.  The plain projections read and write every
    // row below M -- padding rows hold finite values nobody consumes.
    constexpr bool CONV = EPI == EPI_INCONV || EPI == EPI_OUTCONV || EPI == EPI_GENERAL;
    TokMeta tm[NT];
    if constexpr (CONV) {
#pragma unroll
        for (int t = 0; t < NT; ++t) tm[t] = tok_meta(a.blk_win, a.win, tok0 + 16 * t + idx, a.M);
    }
    // transposed-V pass: window and first column (lane group 0) of each of the
    // wave's 16-token blocks, wave-uniform; looked up here so the loads are
    // long done when the epilogue needs them
    int vw[NT], vcol[NT];
    if constexpr (EPI == EPI_QKV) {
        if (swap) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int mb = tok0 + 16 * t;
                vw[t] = mb < a.M ? a.blk_win[mb >> 4] : -1;
                vcol[t] = -1;
                if (vw[t] >= 0) {
                    const int ttb = mb - a.win[vw[t]].tok_off;   // multiple of 16
                    if constexpr (P::kIsBF16 || P::kSplit) vcol[t] = a.win[vw[t]].vt_off + (ttb >> 5) * 32 + 4 * ((ttb >> 4) & 1);
                    else vcol[t] = a.win[vw[t]].vt_off + ttb;
                }
            }
        }
    }

    const int pad = a.taps >> 1;
    const char* wbase = a.W + (size_t)n0 * a.total_groups * 64;
    const int w_row_bytes = a.total_groups * 64;

    auto stage_w = [&](int s_, char* buf) {
        stage_tile<NB * 16, 128, 4>(wbase + (size_t)s_ * 128, (size_t)w_row_bytes, buf, wave, lane);
    };
    // activation fragments of tile s (K-groups 2s, 2s+1)
    auto load_act = [&](int s, u32x4 (&af)[2][NT]) {
#pragma unroll
        for (int kg = 0; kg < 2; ++kg) {
            const int gk = 2 * s + kg;
            const int tap = gk / a.groups_per_tap;
            const int kgi = gk - tap * a.groups_per_tap;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                u32x4 v = u32x4{0u, 0u, 0u, 0u};
                if constexpr (EPI == EPI_GELU) {
                    const int m = tok0 + 16 * t + idx;
                    const int mi = a.stride * m + tap;
                    if (m < a.M && mi < a.M_in && gk < a.real_groups)
                        v = *reinterpret_cast<const u32x4*>(a.act + (size_t)mi * a.lda_bytes + kgi * 64 + g * 16);
                } else if constexpr (CONV) {
                    const int st = tm[t].tt + tap - pad;
                    if (tm[t].w >= 0 && gk < a.real_groups && st >= 0 && st < tm[t].frames) {
                        const int m = tok0 + 16 * t + idx + tap - pad;
                        const char* act = a.act;
                        if constexpr (EPI == EPI_GENERAL) act += (size_t)blockIdx.y * a.act_y_stride;
                        v = *reinterpret_cast<const u32x4*>(act + (size_t)m * a.lda_bytes + kgi * 64 + g * 16);
                    }
                } else {
                    const int m = tok0 + 16 * t + idx;
                    if (m < a.M) v = *reinterpret_cast<const u32x4*>(a.act + (size_t)m * a.lda_bytes + gk * 64 + g * 16);
                }
                af[kg][t] = v;
            }
        }
    };

    f32x4 acc[NB][NT];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[nb][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int steps = a.total_groups >> 1;
    u32x4 acur[2][NT], anext[2][NT];
    stage_w(0, smem);
    load_act(0, acur);
    stamp(1);
    dma_wait_barrier();
    stamp(2);

    // SWAP (V pass of the QKV projection) exchanges the MFMA operands so the
    // accumulator comes out token-major-transposed; compile-time per loop.
    auto main_loop = [&](auto swap_tag) {
        constexpr bool SWAP = decltype(swap_tag)::value;
        for (int s = 0; s < steps; ++s) {
            const bool more = s + 1 < steps;
            if (more) {
                stage_w(s + 1, smem + ((s + 1) & 1) * TILE_BYTES);
                load_act(s + 1, anext);
            }
            const char* buf = smem + (s & 1) * TILE_BYTES;
            // fragment i = (kg, nb) = (i / NB, i % NB)
            using L = FragLayout<128, NB>;
            uint32_t fb[L::VAR];
            L::bases(lds_addr(buf), idx, g, fb);
            lds_stream<L, 2 * NB, (NB >= 8 ? 6 : 3)>(
                fb,
                [&](auto ic, const u32x4& wf) {
                    constexpr int i = decltype(ic)::value;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        mma_kg<P, i / NB, SWAP, 0>(acc[i % NB][t], wf, acur, t, acc[i % NB][t]);
                    }
                });
            if (more) {
#pragma unroll
                for (int kg = 0; kg < 2; ++kg)
#pragma unroll
                    for (int t = 0; t < NT; ++t) acur[kg][t] = anext[kg][t];
            }
            stamp(3 + 2 * s);
            dma_wait_barrier();
            stamp(4 + 2 * s);
        }
    };
    if constexpr (EPI == EPI_QKV) {
        if (swap) main_loop(std::true_type{});
        else main_loop(std::false_type{});
    } else {
        main_loop(std::false_type{});
    }

    // ----------------------------- epilogues --------------------------------
    if constexpr (EPI == EPI_RESLN) {
        // the weight tiles are done with (the loop ended on a barrier): LDS now holds the LN parameters
        float* lnp = reinterpret_cast<float*>(smem);
        stage_params(lnp, a.H, tid, a.bias, a.gamma, a.beta);
        __syncthreads();
        resln<P, NB, NT, LN_EPILOGUE>(acc, lnp, a.X, a.Xb, a.H, tok0, a.M, idx, g);
    } else if constexpr (EPI == EPI_INCONV) {
        // y = live ? PE[tt] + (valid ? conv + bias : 0) : 0.  No control flow around
        // the loads (PE row 0 stands in for dead rows): with the loads inside
        // `if (live)` every (feature block, token block) paid its own global-load
        // latency, 33 k of this kernel's 56 k cycles per workgroup.
        bool live[NT], valid[NT], inside[NT];
        const float* perow[NT];
        PairStore<P> pair[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            live[t] = tm[t].w >= 0 && tm[t].tt < tm[t].frames;
            valid[t] = live[t] && tm[t].tt < tm[t].valid;
            inside[t] = tok0 + 16 * t + idx < a.M;
            perow[t] = a.pe + (size_t)(live[t] ? tm[t].tt : 0) * a.H;
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int n = n0 + pair_feature(nb, g);
            const float4 bv = *reinterpret_cast<const float4*>(a.bias + n);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float4 pv = *reinterpret_cast<const float4*>(perow[t] + n);
                float4 y;
                y.x = live[t] ? pv.x + (valid[t] ? acc[nb][t][0] + bv.x : 0.f) : 0.f;
                y.y = live[t] ? pv.y + (valid[t] ? acc[nb][t][1] + bv.y : 0.f) : 0.f;
                y.z = live[t] ? pv.z + (valid[t] ? acc[nb][t][2] + bv.z : 0.f) : 0.f;
                y.w = live[t] ? pv.w + (valid[t] ? acc[nb][t][3] + bv.w : 0.f) : 0.f;
                if (inside[t]) {
                    const int m = tok0 + 16 * t + idx;
                    if (a.x_tiled == 2)
                        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(a.X) + x16_index(m, n, a.H)) = make_uint2(pack_f16x2(y.x, y.y), pack_f16x2(y.z, y.w));
                    else
                        *reinterpret_cast<float4*>(a.X + (a.x_tiled ? x32_index(m, n, a.H) : (size_t)m * a.H + n)) = y;
                    if constexpr (P::kIsBF16 || P::kSplit) pair[t].put(a.Xb + (size_t)m * a.H * P::kBytes + P::row_byte(n & ~7), nb & 1, y.x, y.y, y.z, y.w);
                }
            }
        }
    } else if constexpr (EPI == EPI_QKV) {
        // The pass's bias values go through LDS (the weight tiles are done with: the loop ended on a barrier).  Read
        // from global memory inside the store loop, every load waited -- vmcnt(0), the compiler's count across the
        // `m < M` control flow -- for the previous block's STORE to be acknowledged (tools/wait_scan.py).
        float* lbias = reinterpret_cast<float*>(smem);
        if (tid < NB * 4) reinterpret_cast<float4*>(lbias)[tid] = reinterpret_cast<const float4*>(a.bias + n0)[tid];
        __syncthreads();
        if (!swap) {
            PairStore<P> pair[NT];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int n = n0 + pair_feature(nb, g);
                const float4 bv = *reinterpret_cast<const float4*>(lbias + pair_feature(nb, g));     // once for all token blocks
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int m = tok0 + 16 * t + idx;
                    if (m >= a.M) continue;
                    pair[t].put(a.out_rows + (size_t)m * a.out_ld * P::kBytes + P::row_byte(n & ~7), nb & 1,
                                acc[nb][t][0] + bv.x, acc[nb][t][1] + bv.y,
                                acc[nb][t][2] + bv.z, acc[nb][t][3] + bv.w);
                }
            }
        } else {
            // swapped operands: lane holds tokens 4g..4g+3 of block t for tile
            // row nb*16 + idx; V^T rows stay in tile order (attn_kernel's
            // output accumulator then owns 8 consecutive head features, see
            // pair_row).  bf16: columns are permuted inside 32-token groups
            // (position 8g + 4e + r, e = parity of the 16-token block) so that
            // the PV A-fragment of attn_kernel is one 16-byte read -- and an
            // (even, odd) block pair of this wave is one 16-byte store.
            bool done_with_previous = false;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (done_with_previous) { done_with_previous = false; continue; }
                if (vw[t] < 0) continue;
                constexpr int kLast = NT - 1;
                const int tn = t < kLast ? t + 1 : t;
                const bool paired = (P::kIsBF16 || P::kSplit) && t < kLast && vw[tn] == vw[t] && (vcol[t] & 4) == 0;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const int row = n0 + nb * 16 + idx;                       // tile row
                    const float bv = lbias[pair_row(nb * 16 + idx)];
                    char* dst = a.vt + (size_t)(row - a.v_start) * a.vt_ld * P::kBytes + P::row_byte(vcol[t] + ((P::kIsBF16 || P::kSplit) ? 8 : 4) * g);
                    if constexpr (P::kSplit) {
                        if (paired) {          // both planes of the 8 columns of the (even, odd) block pair
                            uint32_t h[4], l[4];
                            P::split2(acc[nb][t][0] + bv, acc[nb][t][1] + bv, h[0], l[0]);
                            P::split2(acc[nb][t][2] + bv, acc[nb][t][3] + bv, h[1], l[1]);
                            P::split2(acc[nb][tn][0] + bv, acc[nb][tn][1] + bv, h[2], l[2]);
                            P::split2(acc[nb][tn][2] + bv, acc[nb][tn][3] + bv, h[3], l[3]);
                            *reinterpret_cast<u32x4*>(dst) = u32x4{h[0], h[1], h[2], h[3]};
                            *reinterpret_cast<u32x4*>(dst + 64) = u32x4{l[0], l[1], l[2], l[3]};
                            continue;
                        }
                    }
                    if (paired) {
                        *reinterpret_cast<u32x4*>(dst) = u32x4{
                            P::pack2(acc[nb][t][0] + bv, acc[nb][t][1] + bv), P::pack2(acc[nb][t][2] + bv, acc[nb][t][3] + bv),
                            P::pack2(acc[nb][tn][0] + bv, acc[nb][tn][1] + bv), P::pack2(acc[nb][tn][2] + bv, acc[nb][tn][3] + bv)};
                    } else {
                        store4<P>(dst, acc[nb][t][0] + bv, acc[nb][t][1] + bv, acc[nb][t][2] + bv, acc[nb][t][3] + bv);
                    }
                }
                done_with_previous = paired;
            }
        }
    } else if constexpr (EPI == EPI_GELU) {
        // exact GELU (erf form, torch.nn.functional.gelu default); W rows in paired order: 16-byte stores
        PairStore<P> pair[NT];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int n = n0 + pair_feature(nb, g);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int m = tok0 + 16 * t + idx;
                if (m >= a.M) continue;
                const f32x2 lo = gelu_erf_pair(f32x2{acc[nb][t][0], acc[nb][t][1]}), hi = gelu_erf_pair(f32x2{acc[nb][t][2], acc[nb][t][3]});
                pair[t].put(a.out_rows + (size_t)m * a.out_ld * P::kBytes + P::row_byte(n & ~7), nb & 1, lo.x, lo.y, hi.x, hi.y);
            }
        }
    } else if constexpr (EPI == EPI_GENERAL) {
        // y = act_fn(acc + bias) [zeroed past the window's valid rows] [+ residual] -> fp32 rows and / or 16-bit rows.
        // NB == 16: W rows in paired order (16-byte stores of the 16-bit copy); other NB: plain order, fp32 output only.
        PairStore<P> pair[NT];
        float* lbias = reinterpret_cast<float*>(smem);       // (as EPI_QKV: the bias through LDS)
        if (tid < NB * 4) reinterpret_cast<float4*>(lbias)[tid] = reinterpret_cast<const float4*>(a.bias + n0)[tid];
        __syncthreads();
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int n = n0 + (NB == 16 ? pair_feature(nb, g) : nb * 16 + 4 * g);
            const float4 bv = *reinterpret_cast<const float4*>(lbias + (n - n0));
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int m = tok0 + 16 * t + idx;
                if (m >= a.M) continue;
                float y[4] = {acc[nb][t][0] + bv.x, acc[nb][t][1] + bv.y, acc[nb][t][2] + bv.z, acc[nb][t][3] + bv.w};
                if (a.act_fn == 2) {
                    const f32x2 lo = gelu_erf_pair(f32x2{y[0], y[1]}), hi = gelu_erf_pair(f32x2{y[2], y[3]});
                    y[0] = lo.x; y[1] = lo.y; y[2] = hi.x; y[3] = hi.y;
                } else if (a.act_fn == 1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[r] = fmaxf(y[r], 0.f);
                }
                if (a.zero_invalid && !(tm[t].w >= 0 && tm[t].tt < tm[t].valid)) y[0] = y[1] = y[2] = y[3] = 0.f;
                if (a.residual) {
                    const float4 rv = *reinterpret_cast<const float4*>(a.residual + (size_t)m * a.out_ld32 + n);
                    y[0] += rv.x; y[1] += rv.y; y[2] += rv.z; y[3] += rv.w;
                }
                if (a.out32) *reinterpret_cast<float4*>(a.out32 + (size_t)m * a.out_ld32 + n) = make_float4(y[0], y[1], y[2], y[3]);
                if constexpr (NB == 16) {
                    if (a.out_rows) {
                        if constexpr (P::kIsBF16 || P::kSplit) pair[t].put(a.out_rows + (size_t)m * a.out_ld * P::kBytes + P::row_byte(n & ~7), nb & 1, y[0], y[1], y[2], y[3]);
                        else store4<P>(a.out_rows + ((size_t)m * a.out_ld + n) * P::kBytes, y[0], y[1], y[2], y[3]);
                    }
                }
            }
        }
    } else if constexpr (EPI == EPI_RELU) {
        float* lbias = reinterpret_cast<float*>(smem);       // (as EPI_QKV: no global load between the stores)
        if (tid < NB * 4) reinterpret_cast<float4*>(lbias)[tid] = reinterpret_cast<const float4*>(a.bias + n0)[tid];
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int m = tok0 + 16 * t + idx;
            if (m >= a.M) continue;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int n = n0 + nb * 16 + 4 * g;
                const float4 bv = *reinterpret_cast<const float4*>(lbias + nb * 16 + 4 * g);
                // (split operands: the hi plane's place of the element inside its [32 hi | 32 lo] block)
                char* dst = a.out_rows + (size_t)m * a.out_ld * P::kBytes;
                if constexpr (P::kSplit) dst += P::row_byte(n); else dst += (size_t)n * P::kBytes;
                store4<P>(dst,
                          fmaxf(acc[nb][t][0] + bv.x, 0.f), fmaxf(acc[nb][t][1] + bv.y, 0.f),
                          fmaxf(acc[nb][t][2] + bv.z, 0.f), fmaxf(acc[nb][t][3] + bv.w, 0.f));
            }
        }
    } else if constexpr (EPI == EPI_OUTCONV) {
        // logits = (conv + bias) * mask; per-frame softmax over the out_C
        // phonemes: per-lane partial over (nb, r), then shuffles over g.
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bool live = tm[t].w >= 0 && tm[t].tt < tm[t].frames;
            const bool valid = live && tm[t].tt < tm[t].valid;
            float v[NB][4];
            float mx = -INFINITY, chk = 0.f;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float4 bv = *reinterpret_cast<const float4*>(a.bias + nb * 16 + 4 * g);
                const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = nb * 16 + 4 * g + r;
                    v[nb][r] = valid ? acc[nb][t][r] + bb[r] : 0.f;
                    if (n < a.out_C) mx = fmaxf(mx, v[nb][r]);
                    if (n < a.out_C) chk = fmaf(v[nb][r], 0.f, chk);     // NaN as soon as one logit is NaN or infinite
                }
            }
            if (chk != chk && a.overflow) atomicOr(a.overflow, 1u);
            if (a.softmax) {
                mx = wave_max_g(mx);
                float sum = 0.f;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int n = nb * 16 + 4 * g + r;
                        const float e = (n < a.out_C) ? expf(v[nb][r] - mx) : 0.f;
                        v[nb][r] = e;
                        sum += e;
                    }
                sum = wave_sum_g(sum);
                const float inv = 1.0f / sum;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[nb][r] *= inv;
            }
            if (live) {
                const PpgWindow w = a.win[tm[t].w];
                if (tm[t].tt >= w.keep_lo && tm[t].tt < w.keep_hi) {
                    const int frame = w.out_frame + (tm[t].tt - w.keep_lo);
                    float* o = a.out + (size_t)w.item * a.out_C * a.out_T + frame;
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int n = nb * 16 + 4 * g + r;
                            if (n < a.out_C) o[(size_t)n * a.out_T] = v[nb][r];
                        }
                }
            }
        }
    }
#ifdef PPG_LIN_TIMING
    stamp(13);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stamp(14);
#endif
}

template <class P, int NT, int NB, int EPI>
hipError_t launch_linear_t(const LinearArgs& a, int ypasses, hipStream_t s) {
    if (a.rowmap && NT != 1) return hipErrorInvalidValue;
    const int blocks = a.rowmap ? (a.map_blocks + 3) / 4 : (a.M + 64 * NT - 1) / (64 * NT);
    const size_t lds = 2 * NB * 16 * 128;
    auto kern = linear_kernel<P, NT, NB, EPI>;
    if (lds > 65536) {
        static ppg::LdsLimit limit;
        const hipError_t e = limit.ensure(reinterpret_cast<const void*>(kern), lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(blocks, ypasses), dim3(256), lds, s, a);
    return hipGetLastError();
}

// Token blocks per wave that are built.  `nt` as the product host passes it to ppg::launch_linear (without
// PPG_EXPERIMENT_SWITCHES PpgEngine::lin_nt stays 0 and PPGS_AMD_W2V2_NT / PPGS_AMD_W2V2_POS_NT are not read):
//   ppg_encode, r.lnt (in-conv, qkv, ffn1)                        min(choose_nt(..), 2)
//   ppg_encode, r.lnt_ln (out-proj+LN, ffn2+LN, out-conv)         1
//   ppg_stream.hip (in-conv, qkv, out-proj+LN, out-conv)          1
//   ppg_w2v2_features (EPI_GELU)                                  min(nt, 2)
//   body_forward_one, nt (EPI_GENERAL nb 16, EPI_QKV)             at most 2
//   body_forward_one, pos_nt (EPI_GENERAL nb 3)                   1
// So the product library builds NT 1 and 2 of the wide passes and NT 1 alone of the thin ones (EPI_OUTCONV and the
// 3-block EPI_GENERAL pass); an experiment build has NT 1..3 of both.  What is not built is hipErrorInvalidValue.
#ifdef PPG_EXPERIMENT_SWITCHES
constexpr int kLinWideNt = 3, kLinThinNt = 3;
#else
constexpr int kLinWideNt = 2, kLinThinNt = 1;
#endif

template <class P, int NB, int EPI, int MAXNT>
hipError_t launch_linear_nt(int nt, const LinearArgs& a, int ypasses, hipStream_t s) {
    if (nt == 1) return launch_linear_t<P, 1, NB, EPI>(a, ypasses, s);
    if (nt == 3) {
        if constexpr (MAXNT >= 3) return launch_linear_t<P, 3, NB, EPI>(a, ypasses, s);
        else return hipErrorInvalidValue;
    }
    if constexpr (MAXNT >= 2) return launch_linear_t<P, 2, NB, EPI>(a, ypasses, s);
    else return hipErrorInvalidValue;
}

// Split-precision operands (PrecX2): the token-split kernels of the unfused launch sequence.  Hidden 256: Q/K/V,
// attention, out-projection + LayerNorm, the fused FFN.  Hidden 512 (head dimension 256): the FFN as two GEMMs
// (linear-1 + ReLU into [32 hi | 32 lo] rows, linear-2 + residual + LayerNorm) -- a chunk of the fused FFN kernel
// would have to hold a whole 32-wide hidden group of both weight tiles, 2 x 2 x 64 KiB of LDS.
// (P = PrecX2: a parameter so that only the unit that instantiates it builds these kernels)
template <class P, int NT>
hipError_t launch_linear_x2_nt(int epi, int nb, const LinearArgs& a, int ypasses, hipStream_t s) {
    switch (epi) {
    case EPI_INCONV:  return launch_linear_t<P, NT, 16, EPI_INCONV>(a, ypasses, s);
    case EPI_QKV:     return launch_linear_t<P, NT, 16, EPI_QKV>(a, ypasses, s);
    case EPI_RELU:    return launch_linear_t<P, NT, 16, EPI_RELU>(a, ypasses, s);
    case EPI_GELU:    return launch_linear_t<P, NT, 16, EPI_GELU>(a, ypasses, s);       // wav2vec2 feature encoder
    case EPI_GENERAL: return nb == 16 ? launch_linear_t<P, NT, 16, EPI_GENERAL>(a, ypasses, s) : hipErrorInvalidValue;   // wav2vec2 body
    case EPI_OUTCONV:
        if constexpr (NT <= kLinThinNt) return launch_linear_t<P, NT, 3, EPI_OUTCONV>(a, ypasses, s);
        else return hipErrorInvalidValue;
    case EPI_RESLN:
        if (nb == 16) return launch_linear_t<P, 1, 16, EPI_RESLN>(a, ypasses, s);
        if (nb == 32) return launch_linear_t<P, 1, 32, EPI_RESLN>(a, ypasses, s);
        return hipErrorInvalidValue;
    }
    return hipErrorInvalidValue;
}

}  // namespace

namespace ppg {

// One precision's linear launcher: declared in ppg_linear.hip, instantiated by ppg_linear_<precision>.hip.
template <class P>
hipError_t launch_linear_p(int epi, int nb, int nt, const LinearArgs& a, int ypasses, hipStream_t s) {
    if constexpr (P::kSplit) {
        return nt == 1 ? launch_linear_x2_nt<P, 1>(epi, nb, a, ypasses, s) : launch_linear_x2_nt<P, 2>(epi, nb, a, ypasses, s);
    } else {
        switch (epi) {
        case EPI_INCONV: return launch_linear_nt<P, 16, EPI_INCONV, kLinWideNt>(nt, a, ypasses, s);
        case EPI_QKV:    return launch_linear_nt<P, 16, EPI_QKV, kLinWideNt>(nt, a, ypasses, s);
        case EPI_RELU:   return launch_linear_nt<P, 16, EPI_RELU, kLinWideNt>(nt, a, ypasses, s);
        case EPI_GELU:   return launch_linear_nt<P, 16, EPI_GELU, kLinWideNt>(nt, a, ypasses, s);
        case EPI_GENERAL: return nb == 3 ? launch_linear_nt<P, 3, EPI_GENERAL, kLinThinNt>(nt, a, ypasses, s) : launch_linear_nt<P, 16, EPI_GENERAL, kLinWideNt>(nt, a, ypasses, s);
        case EPI_OUTCONV:return launch_linear_nt<P, 3, EPI_OUTCONV, kLinThinNt>(nt, a, ypasses, s);
        case EPI_RESLN:
            // one 16-token block per wave: the LayerNorm epilogue holds a whole feature row per token in registers
            if (nb == 16) return launch_linear_t<P, 1, 16, EPI_RESLN>(a, ypasses, s);
            if (nb == 32) return launch_linear_t<P, 1, 32, EPI_RESLN>(a, ypasses, s);
            return hipErrorInvalidValue;
        }
        return hipErrorInvalidValue;
    }
}

}  // namespace ppg
