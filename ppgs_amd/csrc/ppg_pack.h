// Weight packing (members of ppg::Packer, ppg_host.h): host fp32 matrices -> device operands in the packer's element
// format, as plain padded matrices or as the MFMA fragment images of the feature-split kernels.
#pragma once

#include "ppg_host.h"

namespace ppg {

// Row of a 32-row block that lane row rho (= lane & 31) of an A fragment holds, where the result's rows go on as
// accumulators: the order in which the 32x32x16 MFMA hands a lane 16 consecutive features (ppg_layer32.h; the head32,
// ffn32x2, gemm32 and posconv kernels share it)
inline int phi(int rho) { return 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3); }
// K index in slot j of lane ln of K-step ks, natural K order: lanes 0..31 hold slots 0..7, lanes 32..63 slots 8..15
inline int frag_k(int ks, int ln, int j) { return 16 * ks + 8 * (ln >> 5) + j; }
// ... where K is the x2 / x1 panel of ppg_layer32.hip (LayerNorm's accumulators, 32 features per K-step pair)
inline int panel_k(int ks, int ln, int j) { return 32 * (ks >> 1) + 16 * (ln >> 5) + 8 * (ks & 1) + j; }
// ... where K is a 128-wide hidden chunk h in the accumulator order of phase A (ppg_layer32.hip, ppg_ffn32x2.hip)
inline int hidden_k(int ks, int ln, int j) { return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * (ln >> 5) + (j & 3); }
// fp32 -> fp16 hi + lo pair (PrecX2, ppg_device.h)
inline void split_f16(float v, uint16_t* hi, uint16_t* lo) { *hi = host_f16(v); *lo = host_f16(v - host_f16_to_f32(*hi)); }

inline int Packer::upload(const void* src, size_t bytes, void** dst) {
    void* p = nullptr;
    HIP_OK(hipMalloc(&p, std::max<size_t>(bytes, 16)));
    allocs.push_back(p);
    HIP_OK(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    *dst = p;
    return PPG_OK;
}

inline int Packer::upload_f32(const float* src, size_t n, size_t n_pad, float** dst) {
    std::vector<float> tmp(std::max(n, n_pad), 0.f);
    memcpy(tmp.data(), src, n * sizeof(float));
    return upload(tmp.data(), tmp.size() * sizeof(float), reinterpret_cast<void**>(dst));
}

// dst[r][c] (rows_pad x cols_pad, zero padded) = get(r, c), in the format `as`
template <class F>
int Packer::matrix(Fmt as, int rows, int cols, int rows_pad, int cols_pad, F get, char** dst) {
    const size_t n = (size_t)rows_pad * cols_pad;
    if (as == Fmt::F16X2) {
        if (cols_pad % 32) return fail(PPG_EINVAL, "split-precision operand rows are multiples of 32 elements (%d)", cols_pad);
        std::vector<uint16_t> tmp(2 * n, 0);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const size_t at = ((size_t)r * cols_pad + (c / 32) * 32) * 2 + (c % 32);
                split_f16(get(r, c), &tmp[at], &tmp[at + 32]);
            }
        return upload(tmp.data(), n * 4, reinterpret_cast<void**>(dst));
    }
    if (as != Fmt::F32) {
        std::vector<uint16_t> tmp(n, 0);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) tmp[(size_t)r * cols_pad + c] = as == Fmt::F16 ? host_f16(get(r, c)) : host_bf16(get(r, c));
        return upload(tmp.data(), n * 2, reinterpret_cast<void**>(dst));
    }
    std::vector<float> tmp(n, 0.f);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) tmp[(size_t)r * cols_pad + c] = get(r, c);
    return upload(tmp.data(), n * 4, reinterpret_cast<void**>(dst));
}

// `frags` fragment images of 64 lanes x 8 elements: element j of lane ln of fragment f = get(f, ln, j)
template <class F>
int Packer::image(int frags, F get, char** dst) {
    return matrix(frags * 64, 8, frags * 64, 8, [&](int r, int j) { return get(r >> 6, r & 63, j); }, dst);
}

// hi + lo fragment images (ppg_ffn32x2.hip): `groups` x 16 fragments of fp32 weights get(group, fragment, lane, j),
// every group as its 16 fp16 hi fragments followed by its 16 lo fragments
template <class F>
int Packer::image_hilo(int groups, F get, char** dst) {
    std::vector<uint16_t> tmp((size_t)groups * 32 * 512);
    for (int g = 0; g < groups; ++g)
        for (int f = 0; f < 16; ++f)
            for (int ln = 0; ln < 64; ++ln)
                for (int j = 0; j < 8; ++j) {
                    const size_t at = ((size_t)g * 32 + f) * 512 + ln * 8 + j;
                    split_f16(get(g, f, ln, j), &tmp[at], &tmp[at + 16 * 512]);
                }
    return upload(tmp.data(), tmp.size() * 2, reinterpret_cast<void**>(dst));
}

// ppg_gemm32.hip's image of an N x K weight matrix: [N / 256][wave][K / 128][rb][8 K-steps] fragments, natural K.
// get(n, n_lane, k): n = the fragment row in accumulator order phi, n_lane = the same lane's row in plain order (the
// V passes of a Q | K | V image, whose accumulators come out transposed)
template <class F>
int gemm32_image(Packer& pk, int N, int K, F get, char** dst) {
    const int chunks = K / 128;
    return pk.image((N / 256) * 4 * chunks * 16, [&](int f, int ln, int j) {
        const int ks = f & 7, rb = (f >> 3) & 1, c = (f >> 4) % chunks, wv = ((f >> 4) / chunks) & 3, p = (f >> 4) / chunks / 4;
        const int n0 = 256 * p + 64 * wv + 32 * rb;
        return get(n0 + phi(ln & 31), n0 + (ln & 31), 128 * c + frag_k(ks, ln, j));
    }, dst);
}

}  // namespace ppg
