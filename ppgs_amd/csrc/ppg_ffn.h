// The fused FFN kernels and the launchers that pick an instantiation.  Included by ppg_ffn_<precision>.hip, which
// instantiate ppg::launch_ffn_p for one precision each; ppg_ffn.hip dispatches on the precision.
#pragma once

#include "ppg_tokensplit.h"

namespace {

// ---------------------------------------------------------------------------
// Fused FFN + residual + LayerNorm:
//   X <- LN(X + W2 relu(W1 x + b1) + b2)
// The 2048-wide hidden never leaves registers: per hidden chunk, phase A
// computes h^T[hid][tok] (C layout: 4 consecutive hid per lane), which after
// ReLU/bf16 packing IS the B fragment of phase B (k-slot permutation folded
// into the host-side packing of W2, see pack_w2 in ppg_engine.hip).
// W1/W2 chunk tiles (32 KiB each) are staged global->regs->LDS.
// ---------------------------------------------------------------------------
// The kernel body for one wave.  NTB = 16-token blocks the wave OWNS (their y
// accumulators, LayerNorms, Q/K/V tail), NTA = blocks whose phase A it computes.
// ROLE 0: NTA == NTB, the plain kernel.  ROLE 1 / 2 (ffn_mixed_kernel): an
// owner of 3 blocks lets its partner wave (owner of 2) compute the phase A of
// its third block, so that both run 5 block-phases per chunk -- h of that
// block travels partner -> owner through LDS once per chunk, its x1 fragments
// owner -> partner once per launch.
// Rows m0 .. m0 + R - 1 (dense partial rows slot0 ..) of the split-hidden FFN: b2 + residual + the partial sums in
// split order, LayerNorm-2, X and its operand copy -- ffn_reduce_ln_kernel's arithmetic, R rows of one wave with all
// their loads in flight together (hidden 256: a lane owns features 4 lane .. + 3 of every row).
// LayerNorm-2 of the split-hidden FFN, per float4 of a row's features: written once, for the reduce pass and for the
// closed-groups kernel's own epilogue (ffn_body), which must give a row the same bits.
__device__ __forceinline__ float ln_quad_sum(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float ln_quad_sq(const float4& v, float mean) {
    const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
    return (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
}
__device__ __forceinline__ float ln_rstd(float sq, int H) { return 1.0f / sqrtf(sq / (float)H + kLnEps); }
__device__ __forceinline__ float4 ln_quad_out(const float4& v, float mean, float rstd, const float4& gv, const float4& ev) {
    return make_float4((v.x - mean) * rstd * gv.x + ev.x, (v.y - mean) * rstd * gv.y + ev.y,
                       (v.z - mean) * rstd * gv.z + ev.z, (v.w - mean) * rstd * gv.w + ev.w);
}

template <class P, int R>
__device__ __forceinline__ void reduce_ln_rows(const FfnArgs& a, int splits, int slot0, int m0, int lane, size_t stride) {
    constexpr int H = 256;
    const int n = lane * 4;
    const float4 bv = *reinterpret_cast<const float4*>(a.b2 + n);
    const float4 gv = *reinterpret_cast<const float4*>(a.gamma + n);
    const float4 ev = *reinterpret_cast<const float4*>(a.beta + n);
    float4 xv[R], p[R][8];
    // the partial rows first: their addresses do not depend on the row map (m0 may still be in flight)
#pragma unroll
    for (int j = 0; j < R; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k)      // (unconditional loads: a split past the last re-reads the last one and is not added)
            p[j][k] = *reinterpret_cast<const float4*>(a.partial + (size_t)min(k, splits - 1) * stride + (size_t)(slot0 + j) * H + n);
#pragma unroll
    for (int j = 0; j < R; ++j) xv[j] = *reinterpret_cast<const float4*>(a.X + (size_t)min(m0 + j, a.M - 1) * H + n);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        // (row map = streaming: the partial sums first, from zero, bias + residual last -- the order in which a workgroup
        // that walks all hidden groups itself adds them (FfnArgs::groups), so that both forms give a row the same bits)
        const float4 rx = make_float4(bv.x + xv[j].x, bv.y + xv[j].y, bv.z + xv[j].z, bv.w + xv[j].w);
        float4 acc = a.rowmap ? make_float4(0.f, 0.f, 0.f, 0.f) : rx;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < splits) { acc.x += p[j][k].x; acc.y += p[j][k].y; acc.z += p[j][k].z; acc.w += p[j][k].w; }
        if (a.rowmap) { acc.x += rx.x; acc.y += rx.y; acc.z += rx.z; acc.w += rx.w; }
        float sum = ln_quad_sum(acc);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
        const float mean = sum / (float)H;
        float sq = ln_quad_sq(acc, mean);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sq += __shfl_xor(sq, off);
        const float4 y = ln_quad_out(acc, mean, ln_rstd(sq, H), gv, ev);
        const int m = m0 + j;
        if (m >= a.M) continue;
        *reinterpret_cast<float4*>(a.X + (size_t)m * H + n) = y;
        if constexpr (P::kIsBF16 || P::kSplit) store4<P>(a.Xb + (size_t)m * H * P::kBytes + P::row_byte(n), y.x, y.y, y.z, y.w);
    }
}

template <class P, int NTA, int NTB, int NBH, bool OP, bool QKV, int ROLE, bool CLOSED = false>
__device__ __forceinline__ void ffn_body(const FfnArgs& a, char* smem, const int tok0) {
    constexpr int NT = NTB;                         // token blocks of everything outside the chunk loop
    constexpr int NTX = NTA > NTB ? NTA : NTB;      // operand fragment sets held
    constexpr int NTL = NTA < NTB ? NTA : NTB;      // blocks whose h is produced and consumed by this wave
    static_assert(ROLE == 0 ? NTA == NTB : (ROLE == 1 ? NTA + 1 == NTB : NTA == NTB + 1), "role");
    static_assert(ROLE == 0 || OP, "the mixed tiling exists for the fused out-projection form only");
    constexpr int H = NBH * 16;
    constexpr int ROW1 = H * P::kBytes;             // W1 tile row bytes
    constexpr int XG = ROW1 / 64;                   // K-groups of x
    constexpr int HC = 32768 / ROW1;                // hidden rows per chunk
    constexpr int HB = HC / 16;                     // hidden 16-blocks per chunk
    constexpr int ROW2 = HC * P::kBytes;            // W2 tile row bytes (128 or 64)
    constexpr int HG = ROW2 / 64;                   // K-groups of phase B per chunk
    // LDS: 2 x {W1 tile 32 KiB, W2 tile 32 KiB} (DMA double buffer) + b1
    char* ldsb1 = smem + 131072;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int idx = lane & 15;
    const int g = lane >> 4;
    // gridDim.y > 1: split-hidden mode for token counts that cannot fill the
    // chip -- this workgroup sums only its 1/gridDim.y of the hidden chunks
    // and writes fp32 partial sums; ffn_reduce_ln_kernel finishes the layer.
    const int NC = a.F / HC / gridDim.y;
    const int c_base = blockIdx.y * NC;

    // LDS: W1 tiles at 0 / 32 KiB, W2 tiles at 64 / 96 KiB, b1 at 128 KiB
    // The sum over hidden chunks is order-free: workgroup b walks the chunks
    // starting at its own offset, so that the CUs of one XCD (b, b+8, b+16, ...)
    // do not all pull the same 64 KiB of weights through the same L2 lines at
    // the same moment.
    const int rot = a.rowmap ? 0 : (blockIdx.x >> 3) % NC;     // (row map = streaming: a recomputed row must give the same bits wherever it lands)
    auto hidden_chunk = [&](int c) { const int r = c + rot; return c_base + (r >= NC ? r - NC : r); };
    auto stage_w1 = [&](int c) {
        stage_tile<HC, ROW1, 4>(a.W1 + (size_t)hidden_chunk(c) * 32768, (size_t)ROW1, smem + (c & 1) * 32768, wave, lane);
    };
    auto stage_w2 = [&](int c) {
        stage_tile<H, ROW2, 4>(a.W2p + (size_t)hidden_chunk(c) * ROW2, (size_t)a.F * P::kBytes, smem + 65536 + (c & 1) * 32768, wave, lane);
    };
    // QKV: transposed-V column (lane group 0) of each of the wave's 16-token
    // blocks, wave-uniform, -1 = padding block; see linear_kernel
    int vw[NT], vcol[NT];
    if constexpr (QKV) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int mb = tok0 + 16 * t;
            vw[t] = mb < a.M ? a.blk_win[mb >> 4] : -1;
            vcol[t] = -1;
            if (vw[t] >= 0) {
                const int ttb = mb - a.win[vw[t]].tok_off;
                if constexpr (P::kIsBF16) vcol[t] = a.win[vw[t]].vt_off + (ttb >> 5) * 32 + 4 * ((ttb >> 4) & 1);
                else vcol[t] = a.win[vw[t]].vt_off + ttb;
            }
        }
    }
    // OP: the W1 double buffer first carries the H/HC tiles of W_o
    constexpr int OT = H / HC;
    static_assert(OT % 2 == 0, "W_o tiles must leave the W1 buffers in phase");
    auto stage_wo = [&](int i) {
        stage_tile<HC, ROW1, 4>(a.Wo + (size_t)i * 32768, (size_t)ROW1, smem + (i & 1) * 32768, wave, lane);
    };
    if constexpr (OP) {
        stage_wo(0);
        stage_w2(0);
        stage_wo(1);
    } else {
        stage_w1(0);
        stage_w2(0);
        if (NC > 1) stage_w1(1);
    }
    for (int i = tid; i < a.F / 4; i += 256)
        reinterpret_cast<float4*>(ldsb1)[i] = reinterpret_cast<const float4*>(a.b1)[i];
    // LayerNorm parameters behind b1: [b2 | gamma2 | beta2] and, with OP, [bo | gamma1 | beta1]
    float* lnp2 = reinterpret_cast<float*>(ldsb1) + a.F;
    float* ldsbq = lnp2 + 3 * H;          // QKV: the next layer's in_proj bias, 3H floats
    float* lnp1 = ldsbq + 3 * H;          // last: dead after LN1, the mixed tiling's h hand-off overlays it
    stage_params(lnp2, H, tid, a.b2, a.gamma, a.beta);
    if constexpr (OP) stage_params(lnp1, H, tid, a.bo, a.g1, a.e1);
    if constexpr (QKV) stage_params(ldsbq, H, tid, a.bq, a.bq + H, a.bq + 2 * H);

    // B fragments of the wave's tokens: x (bf16 copy / fp32 X), or with OP the
    // attention output, replaced by LN1's result below
    const char* actp = OP ? a.ao : ((P::kIsBF16 || P::kSplit) ? a.Xb : reinterpret_cast<const char*>(a.X));
    u32x4 xf[XG][NTX];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int m = tok0 + 16 * t + idx;
#pragma unroll
        for (int kg = 0; kg < XG; ++kg) {
            u32x4 v = u32x4{0u, 0u, 0u, 0u};
            if (m < a.M) v = *reinterpret_cast<const u32x4*>(actp + (size_t)m * ROW1 + kg * 64 + g * 16);
            xf[kg][t] = v;
        }
    }
    // hand-off areas of the mixed tiling: per wave pair (wave & 1), x1 fragments once
    // (in the second W2 buffer, free until chunk 0 stages W2(1)) and the raw fp32 h
    // accumulators of one block per chunk (double buffered; from the LN1 parameters on,
    // which are dead by then)
    const uint32_t xfer_x = lds_addr(smem) + 98304 + (wave & 1) * (XG * 1024) + lane * 16;
    const uint32_t xfer_h = lds_addr(smem) + 131072 + (uint32_t)a.F * 4 + 6 * H * 4 + (wave & 1) * (2 * HB * 1024) + lane * 16;

    f32x4 yacc[NBH][NT];
    if constexpr (!OP) {
#pragma unroll
        for (int nb = 0; nb < NBH; ++nb)
#pragma unroll
            for (int t = 0; t < NT; ++t) yacc[nb][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    using LA = FragLayout<ROW1, HB>;
    using LB = FragLayout<ROW2, NBH>;
    constexpr int RA = XG * HB;          // fragments of phase A
    constexpr int UNITS = HB * NTB;      // pack units (one hidden 16-block of one token block the wave owns)
    constexpr int DEPTH = NTX >= 3 ? 6 : 8;
    const uint32_t lds0 = lds_addr(smem);

    // pack unit u = (hb, t): bias + ReLU on the phase-A accumulator, packed
    // straight into the phase-B B-fragment (see header comment)
    // (ROLE 1: the last owned block's accumulators come from the partner wave: hfar)
    // (the bias is already in hv: it was the C operand of the block's first MFMA; in the
    // 16-bit modes the ReLU runs on the packed pair, one v_pk_max_i16 per two values)
    auto pack_unit = [&](auto uc, f32x4 (&hsrc)[HB][NTA], f32x4 (&hfar)[HB], u32x4 (&hf)[HG][NTB]) {
        constexpr int u = decltype(uc)::value;
        constexpr int hb = u / NTB, t = u % NTB;
        const f32x4 hv = [&] { if constexpr (t < NTL) return hsrc[hb][t]; else return hfar[hb]; }();
        if constexpr (P::kSplit) {
            // (a chunk is ONE 32-wide hidden group: blocks 0, 1 are the two halves of the lane's 8 k-slots; hf[0] the hi
            // plane, hf[1] the lo plane -- the 16-bit path's slot order, so W2 is packed as for the 16-bit modes)
            static_assert(HB == 2 && HG == 2, "split operands: hidden 256 (one 32-wide hidden group per chunk)");
            uint32_t h01, l01, h23, l23;
            P::split2(fmaxf(hv[0], 0.f), fmaxf(hv[1], 0.f), h01, l01);
            P::split2(fmaxf(hv[2], 0.f), fmaxf(hv[3], 0.f), h23, l23);
            if constexpr (hb & 1) { hf[0][t].z = h01; hf[0][t].w = h23; hf[1][t].z = l01; hf[1][t].w = l23; }
            else                  { hf[0][t].x = h01; hf[0][t].y = h23; hf[1][t].x = l01; hf[1][t].y = l23; }
        } else if constexpr (P::kIsBF16) {
            const uint32_t lo = P::relu2(P::pack2(hv[0], hv[1])), hi = P::relu2(P::pack2(hv[2], hv[3]));
            if constexpr (hb & 1) { hf[hb >> 1][t].z = lo; hf[hb >> 1][t].w = hi; }
            else                  { hf[hb >> 1][t].x = lo; hf[hb >> 1][t].y = hi; }
        } else {
            hf[hb][t] = u32x4{__float_as_uint(fmaxf(hv[0], 0.f)), __float_as_uint(fmaxf(hv[1], 0.f)),
                              __float_as_uint(fmaxf(hv[2], 0.f)), __float_as_uint(fmaxf(hv[3], 0.f))};
        }
    };
    // phase A of chunk c: h^T = W1c x^T (fragment i = (kg, hb)); the VALU of
    // `filler(step)` is issued between the MFMAs so the matrix pipe stays fed
    // (destination: rows OFF .. OFF + HB of `dst`, an [..][NT] accumulator array)
    // `cinit`: null -> accumulate from zero; else cinit[hb] is the C operand of block hb's
    // first MFMA (the lane's 4 bias values of the block's rows)
    auto phase_a_into = [&](int c, auto& dst, auto off_tag, auto count_tag, auto cinit, auto filler) {
        constexpr int OFF = decltype(off_tag)::value;
        constexpr int COUNT = decltype(count_tag)::value;       // token blocks
        uint32_t fba[LA::VAR];
        LA::bases(lds0 + (c & 1) * 32768, idx, g, fba);
        lds_stream<LA, RA, DEPTH>(fba, [&](auto ic, const u32x4& wf) {
            constexpr int i = decltype(ic)::value;
#pragma unroll
            for (int t = 0; t < COUNT; ++t) {
                if constexpr (i / HB == 0) {
                    if constexpr (std::is_same_v<decltype(cinit), std::nullptr_t>) mma_kg<P, 0, false, 1>(dst[OFF + i % HB][t], wf, xf, t, dst[OFF + i % HB][t]);
                    else mma_kg<P, 0, false, 2>(dst[OFF + i % HB][t], wf, xf, t, cinit[i % HB]);
                } else mma_kg<P, i / HB, false, 0>(dst[OFF + i % HB][t], wf, xf, t, dst[OFF + i % HB][t]);
            }
            filler(ic);
        });
    };
    auto phase_a = [&](int c, f32x4 (&hdst)[HB][NTA], const f32x4 (&bias)[HB], auto filler) {
        phase_a_into(c, hdst, std::integral_constant<int, 0>{}, std::integral_constant<int, NTA>{}, &bias[0], filler);
    };
    // b1 of hidden chunk c as the lane's C operands (rows 4g .. 4g+3 of each 16-row block)
    auto load_b1 = [&](int c, f32x4 (&bias)[HB]) {
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
            u32x4 raw;
            ds_read_b128_asm<0>(raw, lds_addr(ldsb1) + (hidden_chunk(c) * HC + hb * 16 + 4 * g) * 4);
            bias[hb] = __builtin_bit_cast(f32x4, raw);
        }
    };

#ifdef PPG_FFN_TIMING
    auto pstamp = [&](int k) {
        if (a.dbg && blockIdx.x == 0 && lane == 0) a.dbg[128 + wave * 16 + k] = __builtin_amdgcn_s_memtime();
    };
#else
    auto pstamp = [&](int) {};
#endif
    pstamp(0);
    if constexpr (OP) {
        // x1 = LN1(X + W_o ao + b_o): the out-projection runs like a phase A
        // per W_o tile, straight into the (not yet live) y accumulators; the
        // W_o rows are in paired order, so the accumulators of blocks 2p, 2p+1
        // are K-group p of the next GEMM's B operand (bf16; fp32: W1's columns
        // are uploaded in the matching order).  x1 also stays in the y
        // accumulators: the FFN sums on top of it, so the second residual
        // costs no memory traffic at all.
        float4 res0[NBH];        // LN1's residual rows of block 0: fetched under the last W_o tile's MFMAs
        [&]<int... I>(std::integer_sequence<int, I...>) {
            ([&] {
                dma_wait_barrier();
                pstamp(1 + 2 * I);
                if constexpr (I == OT - 1) load_residual_rows<NBH>(res0, a.X, H, tok0 + idx, a.M, g);
                phase_a_into(I, yacc, std::integral_constant<int, I * HB>{}, std::integral_constant<int, NTB>{}, nullptr, [](auto) {});
                __syncthreads();              // buffer I & 1 is free for the tile after next
                if constexpr (I + 2 < OT) stage_wo(I + 2);
                else if (I + 2 - OT < NC) stage_w1(I + 2 - OT);
                pstamp(2 + 2 * I);
            }(), ...);
        }(std::make_integer_sequence<int, OT>{});
        ln_keep<P, NBH, NT, XG, NTX>(yacc, xf, lnp1, a.X, H, tok0, a.M, idx, g, res0);
        pstamp(12);
        // yacc keeps x1: phase B accumulates W2 h on top of the residual
        if constexpr (ROLE == 1) {
            // the partner computes the phase A of this wave's last block: hand it the fragments
#pragma unroll
            for (int kg = 0; kg < XG; ++kg)
                asm volatile("ds_write_b128 %0, %1" :: "v"(xfer_x + kg * 1024), "v"(xf[kg][NTB - 1]) : "memory");
        }
    }

    // one chunk: [A(c+1) || pack(c)] -> B(c)
#ifdef PPG_FFN_TIMING
    auto stamp = [&](int c, int k) {
        if (a.dbg && blockIdx.x == 0 && lane == 0 && c >= 8 && c < 12)
            a.dbg[(wave * 4 + (c - 8)) * 8 + k] = __builtin_amdgcn_s_memtime();
    };
#else
    auto stamp = [&](int, int) {};
#endif
    // ROLE 2: the raw phase-A accumulators of the partner's block (index NTA - 1 of
    // this wave's phase-A set) for hidden chunk c go to hand-off buffer c & 1; the
    // owner applies bias, ReLU and packing among its own pack units
    auto send_foreign = [&](int c, f32x4 (&hsrc)[HB][NTA]) {
#pragma unroll
        for (int hb = 0; hb < HB; ++hb)
            asm volatile("ds_write_b128 %0, %1" :: "v"(xfer_h + ((c & 1) * HB + hb) * 1024), "v"(hsrc[hb][NTA - 1]) : "memory");
    };
    auto chunk = [&](int c, f32x4 (&hcur)[HB][NTA], f32x4 (&hnext)[HB][NTA]) {
        stamp(c, 0);
        f32x4 b1n[HB];                       // bias of the NEXT chunk: C operands of its phase A
        if (c + 1 < NC) load_b1(c + 1, b1n);
        u32x4 hf[HG][NTB];
        f32x4 hfar[HB];
        if constexpr (ROLE == 1) {
            // raw h of the last block for this chunk: written by the partner before the barrier that ended chunk c - 1
#pragma unroll
            for (int hb = 0; hb < HB; ++hb) {
                u32x4 raw;
                ds_read_b128_asm<0>(raw, xfer_h + ((c & 1) * HB + hb) * 1024);
                hfar[hb] = __builtin_bit_cast(f32x4, raw);
            }
        }
        if (c + 2 < NC) stage_w1(c + 2);
        if (c + 1 < NC) stage_w2(c + 1);
        stamp(c, 1);
        if (c + 1 < NC) {
            // (stream step 0 waits on an LDS op younger than the b1 / hand-off reads above)
            phase_a(c + 1, hnext, b1n, [&](auto ic) {
                constexpr int i = decltype(ic)::value;
                if constexpr (i == 0 && ROLE == 1) {
#pragma unroll
                    for (int hb = 0; hb < HB; ++hb) asm volatile("" : "+v"(hfar[hb]));
                }
                // spread the UNITS pack units evenly over the RA stream steps
                if constexpr ((i * UNITS) / RA != ((i + 1) * UNITS) / RA)
                    pack_unit(std::integral_constant<int, (i * UNITS) / RA>{}, hcur, hfar, hf);
            });
            if constexpr (ROLE == 2) send_foreign(c + 1, hnext);
        } else {
            if constexpr (ROLE == 1) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int hb = 0; hb < HB; ++hb) asm volatile("" : "+v"(hfar[hb]));
            }
            [&]<int... U>(std::integer_sequence<int, U...>) {
                (pack_unit(std::integral_constant<int, U>{}, hcur, hfar, hf), ...);
            }(std::make_integer_sequence<int, UNITS>{});
        }
        stamp(c, 2);
        // phase B: y^T += W2c h^T ; fragment i = (kg, nb)
        uint32_t fbb[LB::VAR];
        LB::bases(lds0 + 65536 + (c & 1) * 32768, idx, g, fbb);
        lds_stream<LB, HG * NBH, DEPTH>(fbb, [&](auto ic, const u32x4& wf) {
            constexpr int i = decltype(ic)::value;
#pragma unroll
            for (int t = 0; t < NT; ++t) mma_kg<P, i / NBH, false, 0>(yacc[i % NBH][t], wf, hf, t, yacc[i % NBH][t]);
        });
        stamp(c, 3);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp(c, 4);
        __syncthreads();
        stamp(c, 5);
    };

    // Closed groups (FfnArgs::groups; row-mapped launches of 16 tokens per wave): the accumulator is closed every
    // `group_len` chunks -- added to `ysum` and zeroed -- so that ysum is built exactly as ffn_reduce_ln_kernel builds it from
    // the partial rows of `groups` hidden splits, each of which sums its chunks from zero in this order.
    // It is an instantiation of its own (ffn_closed_kernel): compiled into the plain kernel, the second accumulator cost the
    // small steps, which never use it, 3 .. 4 % of a step.
    constexpr bool GROUPS = CLOSED;
    static_assert(!CLOSED || (!OP && NT == 1 && NBH == 16 && ROLE == 0), "closed groups: the plain 16-token kernel at hidden 256");
    f32x4 ysum[GROUPS ? NBH : 1];
    const int group_len = GROUPS ? NC / max(a.groups, 1) : 0;
    if constexpr (GROUPS) {
#pragma unroll
        for (int nb = 0; nb < NBH; ++nb) ysum[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    int group_left = group_len;

    f32x4 h0[HB][NTA], h1[HB][NTA];
    pstamp(13);
    dma_wait_barrier();
    pstamp(14);
    if constexpr (ROLE == 2) {
        // x1 fragments of the partner's block (written before the barrier above)
#pragma unroll
        for (int kg = 0; kg < XG; ++kg) ds_read_b128_asm<0>(xf[kg][NTA - 1], xfer_x + kg * 1024);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int kg = 0; kg < XG; ++kg) asm volatile("" : "+v"(xf[kg][NTA - 1]));
    }
    {
        f32x4 b10[HB];
        load_b1(0, b10);
        phase_a(0, h0, b10, [](auto) {});
    }
    if constexpr (ROLE == 2) send_foreign(0, h0);
    __syncthreads();                      // W1 buffer 0 is re-filled by chunk 0's DMA; hand-off 0 is written
    for (int c = 0; c < NC; ++c) {
        chunk(c, h0, h1);
#pragma unroll
        for (int hb = 0; hb < HB; ++hb)
#pragma unroll
            for (int t = 0; t < NTA; ++t) h0[hb][t] = h1[hb][t];
        if constexpr (GROUPS) {
            if (group_len > 0 && --group_left == 0) {
                group_left = group_len;
#pragma unroll
                for (int nb = 0; nb < NBH; ++nb) {
                    ysum[nb] += yacc[nb][0];
                    yacc[nb][0] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
    }

    pstamp(9);
    if constexpr (CLOSED) {
        // The reduce pass's arithmetic on the closed sums, in this kernel's layout: bias + residual last, the row's 64
        // float4 sums added in the reduce pass's butterfly order -- its lane q holds features 4 q .. 4 q + 3 and pairs q
        // with q ^ 32, 16, .. 1; here float4 q = 8 (nb >> 1) + 2 g + (nb & 1), so that is nb ^ 8, 4, 2 inside the lane, the
        // lane groups g ^ 2 and g ^ 1 (lanes ^ 32, ^ 16), and nb ^ 1 last.  No partial row, no reduce launch.
        const int m = tok0 + idx;
        const bool ok = m < a.M;
        const float* xrow = a.X + (size_t)(ok ? m : 0) * H;
        float4 v[NBH];
#pragma unroll
        for (int nb = 0; nb < NBH; ++nb) {
            const int n = pair_feature(nb, g);
            const float4 bv = *reinterpret_cast<const float4*>(lnp2 + n);
            const float4 xv = *reinterpret_cast<const float4*>(xrow + n);
            const float4 rx = make_float4(bv.x + xv.x, bv.y + xv.y, bv.z + xv.z, bv.w + xv.w);
            v[nb] = make_float4(ysum[nb][0] + rx.x, ysum[nb][1] + rx.y, ysum[nb][2] + rx.z, ysum[nb][3] + rx.w);
        }
        auto row_sum = [&](auto quad) {
            float half[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                float s = ((quad(0 + e) + quad(8 + e)) + (quad(4 + e) + quad(12 + e))) + ((quad(2 + e) + quad(10 + e)) + (quad(6 + e) + quad(14 + e)));
                s += __shfl_xor(s, 32);
                s += __shfl_xor(s, 16);
                half[e] = s;
            }
            return half[0] + half[1];
        };
        static_assert(NBH == 16, "the butterfly order above is that of 64 float4 per row");
        const float mean = row_sum([&](int nb) { return ln_quad_sum(v[nb]); }) / (float)H;
        const float rstd = ln_rstd(row_sum([&](int nb) { return ln_quad_sq(v[nb], mean); }), H);
        if (!ok) return;
#pragma unroll
        for (int nb = 0; nb < NBH; ++nb) {
            const int n = pair_feature(nb, g);
            const float4 gv = *reinterpret_cast<const float4*>(lnp2 + H + n);
            const float4 ev = *reinterpret_cast<const float4*>(lnp2 + 2 * H + n);
            const float4 y = ln_quad_out(v[nb], mean, rstd, gv, ev);
            *reinterpret_cast<float4*>(a.X + (size_t)m * H + n) = y;
            if constexpr (P::kIsBF16 || P::kSplit) store4<P>(a.Xb + (size_t)m * H * P::kBytes + P::row_byte(n), y.x, y.y, y.z, y.w);
        }
        return;
    }
    if (a.partial != nullptr) {
        // split-hidden: raw partial sums, [split][token][feature] fp32.  Under a row map the rows are those of the
        // launch's slots, densely (the step's rows lie all over the token space: a split stride of the whole space put
        // every 16-row block of every split on a page of its own -- 30 us of address translation in the reduce pass)
        const int prows = a.rowmap ? (int)gridDim.x * 64 : a.M;
        float* part = a.partial + (size_t)blockIdx.y * prows * H;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int m = tok0 + 16 * t + idx;
            if (m >= a.M) continue;
            const int pm = a.rowmap ? (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + idx : m;
#pragma unroll
            for (int nb = 0; nb < NBH; ++nb) {
                const f32x4 y = yacc[nb][t];
                *reinterpret_cast<float4*>(part + (size_t)pm * H + pair_feature(nb, g)) = make_float4(y[0], y[1], y[2], y[3]);
            }
        }
        if constexpr (NT == 1 && NBH == 16 && !OP) {
            if (a.tickets != nullptr) {
                // one-pass form: every workgroup of the tile publishes its partial rows (device-scope release) and draws
                // a ticket; the last one to arrive sees all of them (acquire) and finishes the tile's 64 rows
                __threadfence();
                __syncthreads();
                int* last = reinterpret_cast<int*>(smem);            // (the weight buffers are dead)
                if (tid == 0) {
                    const int drawn = atomicAdd(a.tickets + blockIdx.x, 1);
                    *last = drawn == (int)gridDim.y - 1;
                    if (*last) a.tickets[blockIdx.x] = 0;            // for the next launch
                }
                __syncthreads();
                if (!*last) return;
                __threadfence();
                const int slot0 = (blockIdx.x * 4 + wave) * 16;
                if (tok0 + 16 <= a.M) {
#pragma unroll 1
                    for (int r = 0; r < 16; r += 4) reduce_ln_rows<P, 4>(a, (int)gridDim.y, slot0 + r, tok0 + r, lane, (size_t)prows * H);
                } else {
                    for (int r = 0; r < 16 && tok0 + r < a.M; ++r) reduce_ln_rows<P, 1>(a, (int)gridDim.y, slot0 + r, tok0 + r, lane, (size_t)prows * H);
                }
            }
        }
        return;
    }
    // (OP: nothing derived from the lane coordinates before the chunk loop may stay live across it)
    int tok0e = tok0, idxe = idx, ge = g;
    if constexpr (OP) {
        asm volatile("" : "+v"(tok0e), "+v"(idxe), "+v"(ge));
        tok0e = __builtin_amdgcn_readfirstlane(tok0e);
    }
    if constexpr (!QKV) {
        resln<P, NBH, NT, OP ? LN_NO_RESIDUAL : LN_EPILOGUE>(yacc, lnp2, a.X, a.Xb, H, tok0e, a.M, idxe, ge);
    } else {
        // ---- the next layer's Q/K/V projection on x2 = LN2(...) ----------------
        // x2 is in the accumulators in paired feature order, i.e. (as in the OP
        // prologue) already the B fragments of a GEMM over the hidden dimension.
        // W_qkv streams through the four now idle 32 KiB weight buffers, three
        // tiles of HC rows ahead; every tile yields HC finished features that are
        // stored at once (Q/K rows: 16-byte stores; V tiles: swapped operands,
        // transposed store, see linear_kernel).  With one wave per SIMD the
        // stores are issue-bound (~280 cycles each, measured) and do not overlap
        // the MFMAs -- interleaving them into the next tile's stream changes
        // nothing -- but the tail still beats the stand-alone projection kernel:
        // no activation reload, no second pass over X as bf16.
        static_assert(OP, "the Q/K/V tail needs the residual-in-accumulator form");
        constexpr int QT = 3 * H / HC;                     // W_qkv tiles
        constexpr int PIECES = 32768 / 1024 / 4;           // DMA instructions per tile and wave
        // workgroup b walks the tiles from its own offset (the stores of the
        // lockstepped workgroups then spread over the Q|K row instead of all
        // hitting one 128-byte column)
        const int qrot = blockIdx.x % QT;
        auto tile_of = [&](int i) { const int r = i + qrot; return r >= QT ? r - QT : r; };
        auto stage_q = [&](int i) {
            stage_tile<HC, ROW1, 4>(a.Wq + (size_t)tile_of(i) * 32768, (size_t)ROW1, smem + (i & 3) * 32768, wave, lane);
        };
        // the chunk loop ended on a barrier: all four buffers are free
        stage_q(0); stage_q(1); stage_q(2);
        resln<P, NBH, NT, LN_NO_RESIDUAL_KEEP>(yacc, lnp2, a.X, nullptr, H, tok0e, a.M, idxe, ge);
        pstamp(10);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int kg = 0; kg < XG; ++kg) {
                if constexpr (P::kIsBF16) {
                    xf[kg][t] = u32x4{P::pack2(yacc[2 * kg][t][0], yacc[2 * kg][t][1]), P::pack2(yacc[2 * kg][t][2], yacc[2 * kg][t][3]),
                                      P::pack2(yacc[2 * kg + 1][t][0], yacc[2 * kg + 1][t][1]), P::pack2(yacc[2 * kg + 1][t][2], yacc[2 * kg + 1][t][3])};
                } else {
                    xf[kg][t] = u32x4{__float_as_uint(yacc[kg][t][0]), __float_as_uint(yacc[kg][t][1]),
                                      __float_as_uint(yacc[kg][t][2]), __float_as_uint(yacc[kg][t][3])};
                }
            }
        }
        bool full_rows = true, full_cols = true;           // every store below is really issued: counted waits are exact
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            full_rows = full_rows && tok0 + 16 * t < a.M;
            full_cols = full_cols && vcol[t] >= 0;
        }
        const int v_start = 2 * H;
#ifdef PPG_FFN_TIMING
        auto qstamp = [&](int i, int k) {
            if (a.dbg && blockIdx.x == 0 && lane == 0 && wave == 0 && i >= 4 && i < 10) a.dbg[192 + (i - 4) * 8 + k] = __builtin_amdgcn_s_memtime();
        };
#else
        auto qstamp = [&](int, int) {};
#endif
        for (int i = 0; i < QT; ++i) {
            qstamp(i, 0);
            // Tile i's DMA is older than: the DMA of tiles i+1, i+2 and the stores of
            // tiles i-2, i-1 (order per iteration: wait, barrier, MFMAs, stores, DMA
            // of tile i+3).  Q/K tiles store HB/2 * NT times per wave, V tiles at
            // least as often, so that many operations may stay in flight.
            constexpr int NSTORE = (HB / 2 > 0 ? HB / 2 : 1) * NT;
            if (full_rows && full_cols && i >= 2 && i + 2 < QT)
                asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * PIECES + 2 * NSTORE) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            qstamp(i, 1);
            __syncthreads();
            qstamp(i, 2);
            const int n0 = tile_of(i) * HC;
            const bool swap = n0 >= v_start;
            f32x4 acc[HB][NT];
            uint32_t fba[LA::VAR];
            LA::bases(lds0 + (i & 3) * 32768, idx, g, fba);
            auto mfmas = [&](auto swap_tag) {
                constexpr bool SWAP = decltype(swap_tag)::value;
                lds_stream<LA, RA, DEPTH>(fba, [&](auto ic, const u32x4& wf) {
                    constexpr int f = decltype(ic)::value;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        if constexpr (f / HB == 0) {
                            if constexpr (SWAP) P::mma0(acc[f % HB][t], xf[0][t], wf);
                            else P::mma0(acc[f % HB][t], wf, xf[0][t]);
                        } else {
                            if constexpr (SWAP) P::mma(acc[f % HB][t], xf[f / HB][t], wf);
                            else P::mma(acc[f % HB][t], wf, xf[f / HB][t]);
                        }
                    }
                });
            };
            if (!swap) {
                mfmas(std::false_type{});
                qstamp(i, 3);
                PairStore<P> pair[NT];
#pragma unroll
                for (int nb = 0; nb < HB; ++nb) {
                    const int gb = n0 / 16 + nb;                     // 16-row block index in W_qkv
                    const int n = pair_feature(gb, g);
                    const float4 bv = *reinterpret_cast<const float4*>(ldsbq + n);
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int m = tok0 + 16 * t + idx;
                        if (tok0 + 16 * t >= a.M) continue;          // wave-uniform
                        pair[t].put(a.qk_out + ((size_t)m * 2 * H + (n & ~7)) * P::kBytes, gb & 1,
                                    acc[nb][t][0] + bv.x, acc[nb][t][1] + bv.y,
                                    acc[nb][t][2] + bv.z, acc[nb][t][3] + bv.w);
                    }
                }
            } else {
                mfmas(std::true_type{});
                qstamp(i, 3);
                bool done_with_previous = false;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (done_with_previous) { done_with_previous = false; continue; }
                    if (vw[t] < 0) continue;
                    constexpr int kLast = NT - 1;
                    const int tn = t < kLast ? t + 1 : t;
                    const bool paired = P::kIsBF16 && t < kLast && vw[tn] == vw[t] && (vcol[t] & 4) == 0;
#pragma unroll
                    for (int nb = 0; nb < HB; ++nb) {
                        const int row = n0 + nb * 16 + idx;
                        const float bv = ldsbq[pair_row(row)];
                        char* dst = a.vt_out + ((size_t)(row - v_start) * a.vt_ld + vcol[t] + (P::kIsBF16 ? 8 : 4) * g) * P::kBytes;
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
            qstamp(i, 4);
            if (i + 3 < QT) stage_q(i + 3);       // into the buffer tile i-1 was read from (all waves passed this iteration's barrier)
            qstamp(i, 5);
        }
        pstamp(11);
    }
}

template <class P, int NT, int NBH, bool OP, bool QKV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void ffn_kernel(FfnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tok0 = a.rowmap ? __builtin_amdgcn_readfirstlane(a.rowmap[blockIdx.x * 4 + wave]) : (blockIdx.x * 4 + wave) * 16 * NT;
    ffn_body<P, NT, NT, NBH, OP, QKV, 0>(a, smem, tok0);
}

// The closed-groups form of the 16-token kernel at hidden 256 (FfnArgs::groups): row-mapped launches of big stream steps.
template <class P>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void ffn_closed_kernel(FfnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tok0 = __builtin_amdgcn_readfirstlane(a.rowmap[blockIdx.x * 4 + wave]);
    ffn_body<P, 1, 1, 16, false, false, 0, true>(a, smem, tok0);
}

// Mixed tiling: 160 tokens per workgroup = waves owning 3, 3, 2, 2 blocks of 16,
// with the 2-block waves computing the phase A of their partner's third block
// (ffn_body ROLE 1 / 2): every wave runs 5 block-phases per chunk instead of 6.
// At the benchmark shape (40 960 token rows on 256 CUs = 160 rows per CU) this is
// one workgroup on every CU where 192-token workgroups leave 42 CUs idle.
template <class P, int NBH, bool QKV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void ffn_mixed_kernel(FfnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int base = blockIdx.x * 160;
    if (wave < 2) ffn_body<P, 2, 3, NBH, true, QKV, 1>(a, smem, base + wave * 48);
    else ffn_body<P, 3, 2, NBH, true, QKV, 2>(a, smem, base + 96 + (wave - 2) * 32);
}

// Second half of the split-hidden FFN: X <- LN(X + b2 + sum_s partial[s]).
// One wave per token row (64 lanes x float4 = 256 features; hidden 512 in two
// steps), HBM-bound elementwise.
template <class P>
__global__ __launch_bounds__(256) void ffn_reduce_ln_kernel(FfnArgs a, int splits) {
    const int lane = threadIdx.x & 63;
    // (wave-uniform by construction; said so, the row-map entry is a scalar load -- it does not queue behind the
    // vector loads of the partial sums, which return in issue order)
    const int slot = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = a.rowmap ? a.rowmap[slot >> 4] + (slot & 15) : slot;          // (row map: only the rows of the step)
    if (a.H == 256 && splits <= 8) {
        // (the row-map entry and the partial rows travel together; a row past M is computed and not stored)
        reduce_ln_rows<P, 1>(a, splits, a.rowmap ? slot : min(slot, a.M - 1), m, lane,
                             (size_t)(a.rowmap ? (a.map_blocks + 3) / 4 * 64 : a.M) * 256);
        return;
    }
    if (m >= a.M) return;
    const int H = a.H;
    float4 v[2];
    float sum = 0.f;
    for (int h = 0; h < H / 256; ++h) {
        const int n = h * 256 + lane * 4;
        const float4 bv = *reinterpret_cast<const float4*>(a.b2 + n);
        const float4 xv = *reinterpret_cast<const float4*>(a.X + (size_t)m * H + n);
        const float4 rx = make_float4(bv.x + xv.x, bv.y + xv.y, bv.z + xv.z, bv.w + xv.w);
        float4 acc = a.rowmap ? make_float4(0.f, 0.f, 0.f, 0.f) : rx;      // (row map: bias + residual last, see reduce_ln_rows)
        // the partial sums are added in split order, loaded 8 / 4 / 1 at a time:
        // one load latency per batch instead of one per split
        const float* part = a.partial + (size_t)(a.rowmap ? slot : m) * H + n;
        const size_t stride = (size_t)(a.rowmap ? (a.map_blocks + 3) / 4 * 64 : a.M) * H;
        int sidx = 0;
        auto batch = [&](auto count) {
            constexpr int N = decltype(count)::value;
            for (; sidx + N <= splits; sidx += N) {
                float4 p[N];
#pragma unroll
                for (int j = 0; j < N; ++j) p[j] = *reinterpret_cast<const float4*>(part + (size_t)(sidx + j) * stride);
#pragma unroll
                for (int j = 0; j < N; ++j) { acc.x += p[j].x; acc.y += p[j].y; acc.z += p[j].z; acc.w += p[j].w; }
            }
        };
        batch(std::integral_constant<int, 8>{});
        batch(std::integral_constant<int, 4>{});
        batch(std::integral_constant<int, 1>{});
        if (a.rowmap) { acc.x += rx.x; acc.y += rx.y; acc.z += rx.z; acc.w += rx.w; }
        v[h] = acc;
        sum += ln_quad_sum(acc);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    const float mean = sum / (float)H;
    float sq = 0.f;
    for (int h = 0; h < H / 256; ++h) sq += ln_quad_sq(v[h], mean);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sq += __shfl_xor(sq, off);
    const float rstd = ln_rstd(sq, H);
    for (int h = 0; h < H / 256; ++h) {
        const int n = h * 256 + lane * 4;
        const float4 gv = *reinterpret_cast<const float4*>(a.gamma + n);
        const float4 ev = *reinterpret_cast<const float4*>(a.beta + n);
        const float4 y = ln_quad_out(v[h], mean, rstd, gv, ev);
        *reinterpret_cast<float4*>(a.X + (size_t)m * H + n) = y;
        if constexpr (P::kIsBF16 || P::kSplit) store4<P>(a.Xb + (size_t)m * H * P::kBytes + P::row_byte(n), y.x, y.y, y.z, y.w);
    }
}

template <class P, int NT, int NBH, bool OP, bool QKV>
hipError_t launch_ffn_t(const FfnArgs& a, hipStream_t s) {
    if (a.rowmap && NT != 1) return hipErrorInvalidValue;
    // (closed groups: one workgroup per token tile walks all chunks; the plain 16-token kernel under a row map has the form)
    if (a.groups > 1 && (NT != 1 || NBH != 16 || OP || !a.rowmap || a.partial || a.splits != 1 || a.tickets || (a.F / (32768 / (a.H * P::kBytes))) % a.groups))
        return hipErrorInvalidValue;
    const dim3 blocks(a.rowmap ? (a.map_blocks + 3) / 4 : (a.M + 64 * NT - 1) / (64 * NT), a.partial ? a.splits : 1);
    auto kern = ffn_kernel<P, NT, NBH, OP, QKV>;
    static ppg::LdsLimit closed_limit;
    ppg::LdsLimit* which = nullptr;
    if constexpr (NT == 1 && NBH == 16 && !OP && !QKV) {
        if (a.groups > 1) { kern = ffn_closed_kernel<P>; which = &closed_limit; }
    }
    const size_t lds = 131072 + (size_t)a.F * 4 + ((OP || QKV) ? 9 : 6) * (size_t)a.H * 4;   // b1, [b2 g2 e2], [bq], [bo g1 e1]
    static ppg::LdsLimit limit;
    hipError_t e = (which ? *which : limit).ensure(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, blocks, dim3(256), lds, s, a);
    e = hipGetLastError();
    if (e != hipSuccess || !a.partial) return e;
    if (a.tickets != nullptr) {
        // (the kernel's one-pass form exists for 16 tokens per wave, hidden 256, no fused out-projection, <= 8 splits)
        if (NT == 1 && NBH == 16 && !OP && a.splits <= 8) return e;
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(ffn_reduce_ln_kernel<P>, dim3(a.rowmap ? a.map_blocks * 4 : (a.M + 3) / 4), dim3(256), 0, s, a, a.splits);
    return hipGetLastError();
}

template <class P, bool QKV>
hipError_t launch_ffn_mixed(const FfnArgs& a, hipStream_t s) {
    if constexpr (!P::kIsBF16) {
        return hipErrorInvalidValue;
    } else {
        if (a.H != 256 || a.partial != nullptr) return hipErrorInvalidValue;
        auto kern = ffn_mixed_kernel<P, 16, QKV>;
        constexpr int HB = 4;                                  // 16-row blocks of a 64-hidden chunk (hidden 256, bf16)
        // hand-off: 2 wave pairs x 2 buffers x HB KiB of raw accumulators, from the LN1 parameters on
        const size_t lds = 131072 + (size_t)a.F * 4 + 6 * (size_t)a.H * 4 + 2 * 2 * HB * 1024;
        static ppg::LdsLimit limit;
        const hipError_t e = limit.ensure(reinterpret_cast<const void*>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3((a.M + 159) / 160), dim3(256), lds, s, a);
        return hipGetLastError();
    }
}

template <class P, bool OP, bool QKV>
hipError_t launch_ffn_op(const FfnArgs& a, int nt, hipStream_t s) {
    if (a.H == 256) {
        if (nt == 1) return launch_ffn_t<P, 1, 16, OP, QKV>(a, s);
        if constexpr (P::kIsBF16) if (nt == 3) return launch_ffn_t<P, 3, 16, OP, QKV>(a, s);
        return launch_ffn_t<P, 2, 16, OP, QKV>(a, s);
    }
    if (a.H == 512) return launch_ffn_t<P, 1, 32, OP, QKV>(a, s);
    return hipErrorInvalidValue;
}

}  // namespace

namespace ppg {

// One precision's FFN launcher: declared in ppg_ffn.hip, instantiated by ppg_ffn_<precision>.hip.
template <class P>
hipError_t launch_ffn_p(const FfnArgs& a, int nt, hipStream_t s) {
    if constexpr (P::kSplit) {
        // split-precision operands: hidden 256, unfused (ppg_linear.h, launch_linear_x2_nt, has the launch sequence)
        if (a.H != 256 || a.Wo != nullptr || a.Wq != nullptr) return hipErrorInvalidValue;
        return nt == 1 ? launch_ffn_t<P, 1, 16, false, false>(a, s) : launch_ffn_t<P, 2, 16, false, false>(a, s);
    } else {
        if (a.Wo != nullptr) {
            if (a.partial != nullptr) return hipErrorInvalidValue;   // every split would redo the out-projection
            if (nt == ppg::kFfnMixedTiling) return a.Wq != nullptr ? launch_ffn_mixed<P, true>(a, s) : launch_ffn_mixed<P, false>(a, s);
            if (a.Wq != nullptr) return launch_ffn_op<P, true, true>(a, nt, s);
            return launch_ffn_op<P, true, false>(a, nt, s);
        }
        if (a.Wq != nullptr) return hipErrorInvalidValue;            // the Q/K/V tail comes with the fused out-projection only
        return launch_ffn_op<P, false, false>(a, nt, s);
    }
}

}  // namespace ppg
