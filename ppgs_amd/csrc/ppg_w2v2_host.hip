// Host side of the wav2vec 2.0 models (kernels: ppg_w2v2.hip, ppg_gemm32.hip, ppg_posconv.hip): the feature encoder
// (ppg_w2v2_*) and the transformer body (ppg_w2v2_body_*): weight packing, workspace layout, launch sequence.
#include "ppg_pack.h"

using namespace ppg;

extern "C" {

// ----------------------------------------------------------------------------
// wav2vec 2.0 feature encoder (w2v2fb representation)
// ----------------------------------------------------------------------------
namespace {
constexpr int kW2vLayers = 7;
const int kW2vKernel[kW2vLayers] = {10, 3, 3, 3, 3, 2, 2};      // transformers Wav2Vec2Config.conv_kernel
const int kW2vStride[kW2vLayers] = {5, 2, 2, 2, 2, 2, 2};       // .conv_stride
constexpr int kW2vChannels = 512;

// frames after each layer and the padded rows per item of each layer's token-major buffer:
// R[l-1] = 2 R[l], so that row m of layer l reads rows 2m + tap of layer l-1 for EVERY item
// (item b starts at row b * R[l]); R[6] = T[6] + 1 rounded up to 32 keeps every row a valid
// output reads inside its own item
struct W2vShape { long T[kW2vLayers]; long R[kW2vLayers]; };
bool w2v_shape(long samples, W2vShape* sh) {
    long t = samples;
    for (int l = 0; l < kW2vLayers; ++l) {
        if (t < kW2vKernel[l]) return false;
        t = (t - kW2vKernel[l]) / kW2vStride[l] + 1;
        sh->T[l] = t;
    }
    sh->R[kW2vLayers - 1] = (sh->T[kW2vLayers - 1] + 1 + 31) / 32 * 32;
    for (int l = kW2vLayers - 2; l >= 0; --l) sh->R[l] = 2 * sh->R[l + 1];
    return true;
}
}  // namespace

struct PpgW2v2 {
    Packer pack;                   // device, operand format, the weights' memory
    int precision = 0, num_cus = 256;
    float* w0 = nullptr;           // (512, 10)
    float* gamma = nullptr;
    float* beta = nullptr;
    char* w[kW2vLayers] = {};      // layers 1..6: [512 rows in paired order][taps * 512], GEMM operand type
    // PPGS_AMD_W2V2_CONV32=1 (experiment): layers 1..6 as plain GEMMs on ppg_gemm32.hip (fragment images of the same
    // weights).  Measured at 16 x 160 080 samples: 1.34 ms against 1.29 ms on linear_kernel<EPI_GELU> -- off.
    char* w_img[kW2vLayers] = {};
    float* zero_bias = nullptr;    // (the layers have no bias)
    bool conv32 = false;
};

int ppg_w2v2_create(const PpgW2v2Weights* wts, int precision, int device, PpgW2v2** out) {
    if (!wts || !out) return fail(PPG_EINVAL, "null argument");
    if (!known_precision(precision)) return fail(PPG_EINVAL, "precision %d", precision);
    if (int rc = use_device(device, "wav2vec2 feature encoder")) return rc;
    std::unique_ptr<PpgW2v2> m(new PpgW2v2());
    Packer& pk = m->pack;
    pk.device = device;
    pk.fmt = operand_format(precision);   // (fp16x2: layers 1..6 with every operand an fp16 hi + lo pair in the fp32 path's byte layout -- PrecX2)
    m->precision = precision;
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, device));
    m->num_cus = prop.multiProcessorCount;
    int rc;
    for (int l = 0; l < kW2vLayers; ++l) if (!wts->conv_weight[l]) return fail(PPG_EINVAL, "conv_weight[%d] is null", l);
    if (!wts->norm_weight || !wts->norm_bias) return fail(PPG_EINVAL, "group-norm parameters are null");
    if ((rc = pk.upload_f32(wts->conv_weight[0], (size_t)kW2vChannels * 10, 0, &m->w0))) return rc;
    if ((rc = pk.upload_f32(wts->norm_weight, kW2vChannels, 0, &m->gamma))) return rc;
    if ((rc = pk.upload_f32(wts->norm_bias, kW2vChannels, 0, &m->beta))) return rc;
    for (int l = 1; l < kW2vLayers; ++l) {
        // torch Conv1d weight (out, in, k) -> [out (paired order)][tap * 512 + in]
        const float* w = wts->conv_weight[l];
        const int k = kW2vKernel[l], C = kW2vChannels;
        rc = pk.matrix(C, k * C, C, k * C,
                       [&](int r, int col) { const int tap = col / C, c = col - tap * C; return w[((size_t)pair_row(r) * C + c) * k + tap]; },
                       &m->w[l]);
        if (rc) return rc;
    }
    m->conv32 = ppg::env_experiment("PPGS_AMD_W2V2_CONV32", m->conv32) != 0;
    if (pk.sz() != 2) m->conv32 = false;
    if (m->conv32) {
        // layers 1..6 as plain GEMMs on the feature-split kernel: output row m reads the k input rows 2 m .. as ONE
        // contiguous run of K = k * 512 elements (rows of the input overlap: lda = 2 rows).  Images as the body's,
        // K index = tap * 512 + channel.
        const int C = kW2vChannels;
        for (int l = 1; l < kW2vLayers; ++l) {
            const float* w = wts->conv_weight[l];
            const int k = kW2vKernel[l];
            rc = gemm32_image(pk, C, k * C, [&](int n, int, int kk) { const int tap = kk / C, ch = kk - tap * C; return w[((size_t)n * C + ch) * k + tap]; }, &m->w_img[l]);
            if (rc) return rc;
        }
        std::vector<float> zeros(C, 0.f);
        if ((rc = pk.upload_f32(zeros.data(), C, 0, &m->zero_bias))) return rc;
    }
    *out = m.release();
    return PPG_OK;
}

void ppg_w2v2_destroy(PpgW2v2* model) { delete model; }

int64_t ppg_w2v2_frames(int64_t samples) {
    W2vShape sh;
    return w2v_shape(samples, &sh) ? sh.T[kW2vLayers - 1] : -1;
}

int ppg_w2v2_workspace_bytes(const PpgW2v2* model, int batch, int64_t samples, size_t* bytes) {
    if (!model || !bytes || batch <= 0) return fail(PPG_EINVAL, "bad argument");
    W2vShape sh;
    if (!w2v_shape(samples, &sh)) return fail(PPG_EINVAL, "%lld samples are too few for the conv stack", (long long)samples);
    const size_t row = (size_t)kW2vChannels * model->pack.sz();
    size_t total = align_up((size_t)batch * 65 * sizeof(double), 256);
    total += align_up((size_t)batch * kW2vChannels * sizeof(float2), 256);
    // (+ 1 row: the last output row of a 3-tap layer reads one row past its input -- a padding row nobody consumes)
    total += align_up(((size_t)batch * sh.R[0] + 1) * row, 256);
    total += align_up(((size_t)batch * sh.R[1] + 1) * row, 256);
    *bytes = total;
    return PPG_OK;
}

int ppg_w2v2_features(PpgW2v2* model, const float* audio, int batch, int64_t samples, float* out,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!model || !audio || !out || !workspace) return fail(PPG_EINVAL, "null argument");
    size_t need = 0;
    int rc = ppg_w2v2_workspace_bytes(model, batch, samples, &need);
    if (rc) return rc;
    if (workspace_bytes < need) return fail(PPG_EWORKSPACE, "workspace %zu bytes < required %zu", workspace_bytes, need);
    HIP_OK(hipSetDevice(model->pack.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    W2vShape sh;
    w2v_shape(samples, &sh);
    const size_t row = (size_t)kW2vChannels * model->pack.sz();
    char* base = static_cast<char*>(workspace);
    double* moments = reinterpret_cast<double*>(base);
    size_t off = align_up((size_t)batch * 65 * sizeof(double), 256);
    float2* scale_shift = reinterpret_cast<float2*>(base + off);
    off += align_up((size_t)batch * kW2vChannels * sizeof(float2), 256);
    char* bufs[2];
    bufs[0] = base + off;
    off += align_up(((size_t)batch * sh.R[0] + 1) * row, 256);
    bufs[1] = base + off;
    const int prec = model->precision;
    hipError_t he = ppg::launch_w2v2_layer0(prec, audio, batch, samples, sh.T[0], (int)sh.R[0], model->w0, model->gamma, model->beta,
                                            moments, scale_shift, bufs[0], s);
    if (he != hipSuccess) return fail(PPG_EDEVICE, "w2v2 layer 0: %s", hipGetErrorString(he));
    for (int l = 1; l < kW2vLayers; ++l) {
        if (model->conv32 && kW2vStride[l] == 2 && kW2vKernel[l] * kW2vChannels >= 384) {
            Gemm32Args g{};
            g.x = bufs[(l - 1) & 1]; g.lda_bytes = (int)(kW2vStride[l] * row); g.w_img = model->w_img[l]; g.bias = model->zero_bias;
            g.out16 = bufs[l & 1]; g.M = (int)(batch * sh.R[l]); g.N = kW2vChannels; g.K = kW2vKernel[l] * kW2vChannels; g.act_fn = 2;
            he = ppg::launch_gemm32(prec, g, s);
            if (he != hipSuccess) return fail(PPG_EDEVICE, "w2v2 conv layer %d: %s", l, hipGetErrorString(he));
            continue;
        }
        LinearArgs a{};
        a.v_start = INT_MAX;
        a.act = bufs[(l - 1) & 1]; a.lda_bytes = (int)row; a.taps = kW2vKernel[l];
        a.groups_per_tap = kW2vChannels / model->pack.KG();
        a.real_groups = a.total_groups = a.taps * a.groups_per_tap;
        a.W = model->w[l]; a.N = kW2vChannels; a.H = kW2vChannels;
        a.out_rows = bufs[l & 1]; a.out_ld = kW2vChannels;
        a.M = (int)(batch * sh.R[l]); a.M_in = (int)(batch * sh.R[l - 1]); a.stride = kW2vStride[l];
        const int nt = choose_nt(model->num_cus, 0, a.M, 2);
        he = ppg::launch_linear(prec, EPI_GELU, 16, std::min(nt, 2), a, kW2vChannels / 256, s);
        if (he != hipSuccess) return fail(PPG_EDEVICE, "w2v2 conv layer %d: %s", l, hipGetErrorString(he));
    }
    he = ppg::launch_w2v2_output(prec, bufs[(kW2vLayers - 1) & 1], batch, (int)sh.R[kW2vLayers - 1], sh.T[kW2vLayers - 1], out, s);
    if (he != hipSuccess) return fail(PPG_EDEVICE, "w2v2 output: %s", hipGetErrorString(he));
    return PPG_OK;
}

// ----------------------------------------------------------------------------
// wav2vec 2.0 transformer body (include/ppgs_amd.h: ppg_w2v2_body_*): HF Wav2Vec2FeatureProjection,
// Wav2Vec2PositionalConvEmbedding and 12 post-norm encoder layers, one launch per GEMM (a fused layer at
// hidden 768 is bound by the weights a workgroup would stream).  16-bit modes: every projection (feature projection,
// Q | K | V, out-proj, FFN-1, FFN-2) on ppg_gemm32.hip with its epilogue fixed per use, the positional convolution on
// ppg_posconv.hip, LayerNorm-768 as a row kernel, attention as attn_kernel<.., 1, 64> (12 heads of 64).  fp32 mode (and
// the PPGS_AMD_W2V2_* = 0 switches): the same sequence on linear_kernel<EPI_QKV / EPI_GENERAL> (bias, GELU, residual
// in the epilogue; the positional convolution as 16 grouped k-tap GEMMs of one launch).  Token space: item b owns rows
// b R .. b R + frames - 1, R = frames rounded up to 32 (no half-written V^T groups); one attention window per item,
// keys limited to its valid frames.  Batches of >= 8 items run as two half-batches on two HIP streams.
// ----------------------------------------------------------------------------
struct PpgW2v2Body {
    Packer pack;
    int precision = 0, num_cus = 256;
    int hidden = 0, heads = 0, ffn = 0, layers = 0, taps = 0, groups = 0, gpt = 0;
    float eps = 1e-5f;
    float* pn_g = nullptr; float* pn_b = nullptr;
    char* proj_w = nullptr; float* proj_b = nullptr;
    char* proj_img = nullptr;      // the feature projection as gemm32 fragment images (16-bit modes)
    char* pos_w = nullptr; float* pos_b = nullptr;
    char* pos_img = nullptr;       // the positional convolution's fragment image (ppg_posconv.hip, 16-bit modes)
    bool posconv = true;           // PPGS_AMD_W2V2_POSCONV=0: the convolution as a k-tap GEMM on linear_kernel<EPI_GENERAL>
    float* en_g = nullptr; float* en_b = nullptr;
    struct Layer { char* wqkv; float* bqkv; char* wo; float* bo; float* g1; float* e1; char* w1; float* b1; char* w2; float* b2; float* g2; float* e2;
                   char* wo_img; char* w1_img; char* w2_img; char* wqkv_img; };   // fragment images for ppg_gemm32.hip (16-bit modes)
    bool gemm32 = true;            // PPGS_AMD_W2V2_GEMM32=0: linear_kernel<EPI_GENERAL> for every projection
    bool qkv32 = true;             // PPGS_AMD_W2V2_QKV32=0: Q/K/V on linear_kernel<EPI_QKV>
    std::vector<Layer> layer;
    // per pipeline (a batch of >= 8 items runs as two half-batches on two HIP streams, as the PPG network's engine does)
    struct Slot { char* staging = nullptr; size_t staging_bytes = 0; hipEvent_t uploaded = nullptr; };   // pinned tables of the call in flight
    Slot slot[2];
    int pipelines = 2;             // PPGS_AMD_W2V2_STREAMS
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    ~PpgW2v2Body() {
        (void)hipSetDevice(pack.device);
        for (Slot& sl : slot) {
            if (sl.staging) (void)hipHostFree(sl.staging);
            if (sl.uploaded) (void)hipEventDestroy(sl.uploaded);
        }
        if (side) (void)hipStreamDestroy(side);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
    }
};

int ppg_w2v2_body_create(const PpgW2v2BodyWeights* w, int precision, int device, PpgW2v2Body** out) {
    if (!w || !out) return fail(PPG_EINVAL, "null argument");
    if (!known_precision(precision)) return fail(PPG_EINVAL, "precision %d", precision);
    const int H = w->hidden, F = w->ffn, L = w->num_layers;
    if (H != 768 || w->heads <= 0 || H / w->heads != 64 || H % w->heads) return fail(PPG_EINVAL, "hidden %d / heads %d: the body kernels are built for 768 = 12 x 64", H, w->heads);
    if (F <= 0 || F % 256 || L < 0 || L > PPG_W2V2_MAX_LAYERS) return fail(PPG_EINVAL, "ffn %d, layers %d", F, L);
    if (w->conv_groups != 16 || w->conv_kernel <= 0 || w->conv_kernel % 2 || H / w->conv_groups != 48)
        return fail(PPG_EINVAL, "positional convolution: kernel %d groups %d", w->conv_kernel, w->conv_groups);
    if (int rc = use_device(device, "wav2vec2 body")) return rc;
    std::unique_ptr<PpgW2v2Body> m(new PpgW2v2Body());
    Packer& pk = m->pack;
    pk.device = device; m->precision = precision;
    // fp16x2: every projection and the attention on fp16 hi + lo operand pairs (PrecX2: the fp32 path's launch sequence
    // and byte layout, three fp16 MFMAs per product); the positional convolution stays on f32-input MFMAs (its groups
    // of 48 channels are not whole [32 hi | 32 lo] blocks)
    pk.fmt = operand_format(precision);
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, device));
    m->num_cus = prop.multiProcessorCount;
    m->hidden = H; m->heads = w->heads; m->ffn = F; m->layers = L; m->taps = w->conv_kernel; m->groups = w->conv_groups;
    m->eps = w->layer_norm_eps;
    m->gemm32 = ppg::env_switch("PPGS_AMD_W2V2_GEMM32", m->gemm32) != 0;
    m->qkv32 = ppg::env_experiment("PPGS_AMD_W2V2_QKV32", m->qkv32) != 0;
    if (pk.sz() != 2 || H % 256 || F % 256 || H % 128 || F % 128) m->gemm32 = false;
    const int CG = H / w->conv_groups;                       // 48 channels per group
    m->gpt = (CG * pk.sz() + 63) / 64;                         // K-groups of 64 bytes per tap: 2 (16-bit, padded) or 3 (fp32)
    int rc;
#define NEED(ptr) if (!(ptr)) return fail(PPG_EINVAL, #ptr " is null")
    NEED(w->proj_norm_weight); NEED(w->proj_norm_bias); NEED(w->proj_weight); NEED(w->proj_bias);
    NEED(w->pos_conv_weight); NEED(w->pos_conv_bias); NEED(w->enc_norm_weight); NEED(w->enc_norm_bias);
    auto paired = [&](const float* src, int rows, int cols, char** dst) {
        return pk.matrix(rows, cols, rows, cols, [&](int r, int c) { return src[(size_t)pair_row(r) * cols + c]; }, dst);
    };
    if ((rc = pk.upload_f32(w->proj_norm_weight, 512, 0, &m->pn_g))) return rc;
    if ((rc = pk.upload_f32(w->proj_norm_bias, 512, 0, &m->pn_b))) return rc;
    if ((rc = paired(w->proj_weight, H, 512, &m->proj_w))) return rc;
    auto image = [&](const float* src, int N, int K, char** dst) {
        return gemm32_image(pk, N, K, [&](int n, int, int k) { return src[(size_t)n * K + k]; }, dst);
    };
    if (m->gemm32 && (rc = image(w->proj_weight, H, 512, &m->proj_img))) return rc;
    if ((rc = pk.upload_f32(w->proj_bias, H, 0, &m->proj_b))) return rc;
    {   // W'[n][tap * gpt * KG + c] = w[n][c][tap] for c < 48 (n's own group), 0 for the pad channels; plain row order
        // (fp16x2: as plain fp32 -- this one GEMM runs on the f32-input MFMAs)
        const int taps = m->taps, kk = m->gpt * pk.KG();
        const float* pw = w->pos_conv_weight;
        rc = pk.matrix(pk.split() ? Fmt::F32 : pk.fmt, H, taps * kk, H, taps * kk,
                       [&](int n, int col) { const int tap = col / kk, c = col - tap * kk; return c < CG ? pw[((size_t)n * CG + c) * taps + tap] : 0.f; },
                       &m->pos_w);
        if (rc) return rc;
    }
    if ((rc = pk.upload_f32(w->pos_conv_bias, H, 0, &m->pos_b))) return rc;
    m->posconv = ppg::env_switch("PPGS_AMD_W2V2_POSCONV", m->posconv) != 0;
    if (pk.sz() != 2 || w->conv_groups != 16 || CG != 48 || m->taps != 128) m->posconv = false;
    if (m->posconv) {
        const float* pw = w->pos_conv_weight;
        rc = pk.image(16 * 4 * 32 * 6, [&](int f, int ln, int j) {   // ppg_posconv.hip: [group][wave][32 taps][3 K-steps][rb]
            const int rb = f & 1, ks = (f % 6) >> 1, tl = (f / 6) & 31, wv = (f / 192) & 3, g = f / 768;
            const int n = 32 * rb + phi(ln & 31), ch = frag_k(ks, ln, j), tap = 32 * wv + tl;
            return n < CG ? pw[((size_t)(g * CG + n) * CG + ch) * 128 + tap] : 0.f;
        }, &m->pos_img);
        if (rc) return rc;
    }
    if ((rc = pk.upload_f32(w->enc_norm_weight, H, 0, &m->en_g))) return rc;
    if ((rc = pk.upload_f32(w->enc_norm_bias, H, 0, &m->en_b))) return rc;
    m->layer.resize(L);
    for (int l = 0; l < L; ++l) {
        const PpgW2v2LayerWeights& lw = w->layers[l];
        PpgW2v2Body::Layer& d = m->layer[l];
        const float qscale = (float)(1.4426950408889634 / sqrt(64.0));      // 12 heads of 64
        NEED(lw.q_weight); NEED(lw.q_bias); NEED(lw.k_weight); NEED(lw.k_bias); NEED(lw.v_weight); NEED(lw.v_bias);
        NEED(lw.out_weight); NEED(lw.out_bias); NEED(lw.norm1_weight); NEED(lw.norm1_bias);
        NEED(lw.ffn1_weight); NEED(lw.ffn1_bias); NEED(lw.ffn2_weight); NEED(lw.ffn2_bias); NEED(lw.norm2_weight); NEED(lw.norm2_bias);
        // in_proj = [q; k; v] rows, each block of 3H in paired order (linear_kernel<EPI_QKV>)
        rc = pk.matrix(3 * H, H, 3 * H, H,
                       [&](int r, int c) {
                           const int rr = pair_row(r), which = rr / H, row = rr - which * H;
                           const float* src = which == 0 ? lw.q_weight : (which == 1 ? lw.k_weight : lw.v_weight);
                           return src[(size_t)row * H + c] * (which == 0 ? qscale : 1.0f);    // (see ppg_engine_create)
                       }, &d.wqkv);
        if (rc) return rc;
        std::vector<float> bq(3 * (size_t)H);
        for (int i = 0; i < H; ++i) bq[i] = lw.q_bias[i] * qscale;
        memcpy(bq.data() + H, lw.k_bias, H * sizeof(float));
        memcpy(bq.data() + 2 * H, lw.v_bias, H * sizeof(float));
        if ((rc = pk.upload_f32(bq.data(), 3 * (size_t)H, 0, &d.bqkv))) return rc;
        if ((rc = paired(lw.out_weight, H, H, &d.wo))) return rc;
        if ((rc = pk.upload_f32(lw.out_bias, H, 0, &d.bo))) return rc;
        if ((rc = pk.upload_f32(lw.norm1_weight, H, 0, &d.g1))) return rc;
        if ((rc = pk.upload_f32(lw.norm1_bias, H, 0, &d.e1))) return rc;
        if ((rc = paired(lw.ffn1_weight, F, H, &d.w1))) return rc;
        if ((rc = pk.upload_f32(lw.ffn1_bias, F, 0, &d.b1))) return rc;
        if ((rc = paired(lw.ffn2_weight, H, F, &d.w2))) return rc;
        if ((rc = pk.upload_f32(lw.ffn2_bias, H, 0, &d.b2))) return rc;
        if ((rc = pk.upload_f32(lw.norm2_weight, H, 0, &d.g2))) return rc;
        if ((rc = pk.upload_f32(lw.norm2_bias, H, 0, &d.e2))) return rc;
        d.wo_img = d.w1_img = d.w2_img = d.wqkv_img = nullptr;
        if (m->gemm32) {
            // Q | K | V as one image of 3H / 256 passes: Q (scaled as above) and K rows in accumulator order phi, the V
            // passes' rows in pair_row order (their accumulators come out transposed: ppg_gemm32.hip mode 3)
            rc = gemm32_image(pk, 3 * H, H, [&](int n, int n_lane, int k) {
                if (n_lane >= 2 * H) return lw.v_weight[(size_t)pair_row(n_lane - 2 * H) * H + k];
                return n < H ? lw.q_weight[(size_t)n * H + k] * qscale : lw.k_weight[(size_t)(n - H) * H + k];
            }, &d.wqkv_img);
            if (rc) return rc;
            if ((rc = image(lw.out_weight, H, H, &d.wo_img))) return rc;
            if ((rc = image(lw.ffn1_weight, F, H, &d.w1_img))) return rc;
            if ((rc = image(lw.ffn2_weight, H, F, &d.w2_img))) return rc;
        }
    }
#undef NEED
    for (PpgW2v2Body::Slot& sl : m->slot) HIP_OK(hipEventCreateWithFlags(&sl.uploaded, hipEventDisableTiming));
    HIP_OK(hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&m->ev_fork, kForkJoinEventFlags));
    HIP_OK(hipEventCreateWithFlags(&m->ev_join, kForkJoinEventFlags));
    m->pipelines = std::max(1, std::min(ppg::env_switch("PPGS_AMD_W2V2_STREAMS", m->pipelines), 2));
    *out = m.release();
    return PPG_OK;
}

void ppg_w2v2_body_destroy(PpgW2v2Body* body) { delete body; }

namespace {
struct BodyLayout { size_t win, blk, items, ln, x, p, xb, qk, vt, ao, hid, total; int R, M, nitems; };
BodyLayout body_layout(const PpgW2v2Body* m, int batch, int frames) {
    BodyLayout L{};
    const int H = m->hidden, sz = m->pack.sz();
    L.R = round_up(frames, 32);
    L.M = batch * L.R;
    L.nitems = batch * ((frames + 63) / 64);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    L.win = take((size_t)batch * sizeof(PpgWindow));
    L.blk = take((size_t)(L.M / 16) * sizeof(int));
    L.items = take((size_t)L.nitems * sizeof(AttnItem));
    L.ln = take(((size_t)L.M + 1) * 512 * sz);
    L.x = take((size_t)L.M * H * 4);
    L.p = take((size_t)L.M * H * 4);
    L.xb = take(((size_t)L.M + 1) * H * sz + 256);            // (the last group's pad channels read 32 bytes past a row)
    L.qk = take(((size_t)L.M + 64) * 2 * H * sz);
    L.vt = take((size_t)H * (L.M + 64) * sz);
    L.ao = take((size_t)L.M * H * sz);
    L.hid = take((size_t)L.M * m->ffn * sz);
    L.total = off;
    return L;
}

// Items of the first pipeline when the batch is split (0: one pipeline).  Items are independent (one attention
// window each); the projections' 128-row tiles of 8 192 rows are 192 workgroups on 256 CUs, and two half-batches on
// two streams run one half's GEMMs beside the other half's attention and LayerNorm launches.
int body_first_half(const PpgW2v2Body* m, int batch, int frames) {
    const int R = (frames + 31) / 32 * 32;
    if (m->pipelines < 2 || batch < 8 || (long)batch * R < 4096) return 0;
    return (batch + 1) / 2;
}

int body_forward_one(PpgW2v2Body* m, PpgW2v2Body::Slot& slot, const float* features, const int64_t* valid_frames, int batch, int frames,
                     float* out, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const BodyLayout L = body_layout(m, batch, frames);
    if (workspace_bytes < L.total) return fail(PPG_EWORKSPACE, "workspace %zu bytes < required %zu", workspace_bytes, L.total);
    const int H = m->hidden, F = m->ffn, sz = m->pack.sz(), prec = m->precision, M = L.M, R = L.R;
    const bool split = m->pack.split();
    char* base = static_cast<char*>(workspace);

    // tables: one window per item, every 16-row block of item b -> window b, query tiles of 64
    const size_t table_bytes = L.ln;                           // win | blk | items are the first three regions
    if (slot.staging_bytes < table_bytes) {
        if (slot.staging) { HIP_OK(hipEventSynchronize(slot.uploaded)); (void)hipHostFree(slot.staging); slot.staging = nullptr; }
        HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&slot.staging), table_bytes, hipHostMallocDefault));
        slot.staging_bytes = table_bytes;
    }
    HIP_OK(hipEventSynchronize(slot.uploaded));                  // the previous call's upload has left the staging buffer
    memset(slot.staging, 0, table_bytes);
    PpgWindow* hw = reinterpret_cast<PpgWindow*>(slot.staging + L.win);
    int* hb = reinterpret_cast<int*>(slot.staging + L.blk);
    AttnItem* hi = reinterpret_cast<AttnItem*>(slot.staging + L.items);
    int ni = 0;
    for (int b = 0; b < batch; ++b) {
        PpgWindow& w = hw[b];
        w.item = b; w.frames = frames; w.valid = (int)valid_frames[b]; w.keep_lo = 0; w.keep_hi = frames;
        w.tok_off = b * R; w.vt_off = b * R;
        for (int k = 0; k < R / 16; ++k) hb[b * (R / 16) + k] = b;
        for (int q0 = 0; q0 < frames; q0 += 64) hi[ni++] = AttnItem{b, q0, w.tok_off, w.vt_off, frames, w.valid, 0, 0};
    }
    // padding rows, slack rows / columns of the OPERAND buffers: finite (masked keys are still multiplied).  The fp32
    // residual buffers X and P (half of the bytes) are written in full by the projection / every GEMM epilogue.
    HIP_OK(hipMemsetAsync(base + L.ln, 0, L.x - L.ln, s));
    HIP_OK(hipMemsetAsync(base + L.xb, 0, L.hid - L.xb, s));
    HIP_OK(hipMemcpyAsync(base, slot.staging, table_bytes, hipMemcpyHostToDevice, s));
    HIP_OK(hipEventRecord(slot.uploaded, s));
    const PpgWindow* d_win = reinterpret_cast<const PpgWindow*>(base + L.win);
    const int* d_blk = reinterpret_cast<const int*>(base + L.blk);
    const AttnItem* d_items = reinterpret_cast<const AttnItem*>(base + L.items);
    char *ln = base + L.ln, *Xb = base + L.xb, *qk = base + L.qk, *vt = base + L.vt, *ao = base + L.ao, *hid = base + L.hid;
    float *X = reinterpret_cast<float*>(base + L.x), *P = reinterpret_cast<float*>(base + L.p);
    const int vt_ld = M + 64;
    // operand rows of the residual stream: the 16-bit copy (fp16x2: the [32 hi | 32 lo] copy), or X itself in fp32 mode
    const bool op_copy = sz == 2 || split;
    const char* act_x = op_copy ? Xb : reinterpret_cast<const char*>(X);
    char* xb_out = op_copy ? Xb : nullptr;

    // tokens per wave (16 nt).  Measured at 16 x 499 frames, bf16: nt 1 4.41 ms, nt 2 4.82 ms, nt 3 6.35 ms
    int nt = std::min(choose_nt(m->num_cus, 0, M, 2), 2);
    nt = std::max(1, std::min(ppg::env_experiment("PPGS_AMD_W2V2_NT", nt), sz == 2 ? 3 : 2));
    auto general = [&](const char* act, int k_elems, const char* W, const float* bias, int N) {
        LinearArgs a{};
        a.blk_win = d_blk; a.win = d_win; a.M = M; a.H = H; a.v_start = INT_MAX; a.taps = 1;
        a.act = act; a.lda_bytes = k_elems * sz;
        a.groups_per_tap = k_elems / m->pack.KG(); a.real_groups = a.total_groups = a.groups_per_tap;
        a.W = W; a.bias = bias; a.N = N; a.out_ld32 = H;
        return a;
    };
    auto layer_norm = [&](const float* g, const float* b) {
        return ppg::launch_w2v2_layernorm(prec, H, P, nullptr, g, b, M, M, M, m->eps, X, xb_out, s);
    };
    // feature projection: LayerNorm(512) -> Linear, rows past the valid frames zeroed (HF: hidden_states[~mask] = 0)
    LAUNCH_OK(ppg::launch_w2v2_layernorm(prec, 512, features, nullptr, m->pn_g, m->pn_b, (long)batch * frames, frames, R, m->eps,
                                         op_copy ? nullptr : reinterpret_cast<float*>(ln), op_copy ? ln : nullptr, s), "w2v2 projection LayerNorm");
    if (m->gemm32) {
        // (linear_kernel's 16-token waves re-read the 768 x 512 weights per 64 rows: 205 us for 6.4 GFLOP)
        Gemm32Args g{};
        g.x = ln; g.w_img = m->proj_img; g.bias = m->proj_b; g.out32 = X; g.out16 = Xb; g.M = M; g.N = H; g.K = 512;
        g.win = d_win; g.rows_per_item = R;
        LAUNCH_OK(ppg::launch_gemm32(prec, g, s), "w2v2 projection");
    } else {
        LinearArgs a = general(ln, 512, m->proj_w, m->proj_b, H);
        a.zero_invalid = 1; a.out32 = X; a.out_rows = xb_out; a.out_ld = H;
        LAUNCH_OK(ppg::launch_linear(prec, EPI_GENERAL, 16, nt, a, H / 256, s), "w2v2 projection");
    }
    {   // positional convolution (+GELU) + residual -> P, then the encoder's LayerNorm
        if (m->posconv) {
            PosConvArgs pc{};
            pc.x16 = Xb; pc.ldx_bytes = H * 2; pc.w_img = m->pos_img; pc.bias = m->pos_b; pc.residual = X; pc.out32 = P;
            pc.M = M; pc.H = H; pc.rows_per_item = R; pc.frames = frames; pc.tiles_per_item = (R + 127) / 128;
            LAUNCH_OK(ppg::launch_posconv(prec, pc, batch, s), "w2v2 positional convolution");
            LAUNCH_OK(layer_norm(m->en_g, m->en_b), "w2v2 encoder LayerNorm");
        } else {
        // (fp16x2: fp32 rows of X against the fp32 weights, on the f32-input MFMAs)
        LinearArgs a = general(split ? reinterpret_cast<const char*>(X) : act_x, H, m->pos_w, m->pos_b, H);
        a.taps = m->taps; a.groups_per_tap = m->gpt; a.real_groups = a.total_groups = m->taps * m->gpt;
        a.act_y_stride = (H / m->groups) * sz; a.act_fn = 2; a.residual = X; a.out32 = P;
        // (32 or 48 tokens per wave -- fewer re-reads of a group's 590 KB of weights -- measured: no faster, 3.20 / 3.24
        // against 3.23 ms per forward: the launch is bound by the re-reads of the ACTIVATION rows, one pass per tap)
        int pos_nt = 1;
        pos_nt = std::max(1, std::min(ppg::env_experiment("PPGS_AMD_W2V2_POS_NT", pos_nt), sz == 2 ? 3 : 2));
        LAUNCH_OK(ppg::launch_linear(split ? PPG_PRECISION_FP32 : prec, EPI_GENERAL, 3, pos_nt, a, m->groups, s), "w2v2 positional convolution");
        LAUNCH_OK(layer_norm(m->en_g, m->en_b), "w2v2 encoder LayerNorm");
        }
    }
    for (int l = 0; l < m->layers; ++l) {
        const PpgW2v2Body::Layer& d = m->layer[l];
        {
            LinearArgs a = general(act_x, H, d.wqkv, d.bqkv, 3 * H);
            a.out_rows = qk; a.out_ld = 2 * H; a.vt = vt; a.vt_ld = vt_ld; a.v_start = 2 * H;
            if (m->gemm32 && m->qkv32) {
                Gemm32Args g{};
                g.x = Xb; g.w_img = d.wqkv_img; g.bias = d.bqkv; g.out16 = qk; g.M = M; g.N = 3 * H; g.K = H;
                g.vt = vt; g.vt_ld = vt_ld; g.ld_out = 2 * H; g.v_pass0 = 2 * H / 256; g.rows_per_item = R;
                LAUNCH_OK(ppg::launch_gemm32(prec, g, s), "w2v2 qkv");
            } else {
                LAUNCH_OK(ppg::launch_linear(prec, EPI_QKV, 16, nt, a, 3 * H / 256, s), "w2v2 qkv");
            }
        }
        LAUNCH_OK(ppg::launch_attn(prec, attn_args(sz, H, m->heads, 0, qk, vt, vt_ld, ao, d_items, d_win, M), ni, m->heads, 64, s), "w2v2 attention");
        if (m->gemm32) {
            Gemm32Args g{};
            g.x = ao; g.w_img = d.wo_img; g.bias = d.bo; g.residual = X; g.out32 = P; g.M = M; g.N = H; g.K = H;
            LAUNCH_OK(ppg::launch_gemm32(prec, g, s), "w2v2 out-proj");
            LAUNCH_OK(layer_norm(d.g1, d.e1), "w2v2 LayerNorm 1");
            Gemm32Args f1{};
            f1.x = Xb; f1.w_img = d.w1_img; f1.bias = d.b1; f1.out16 = hid; f1.M = M; f1.N = F; f1.K = H; f1.act_fn = 2;
            LAUNCH_OK(ppg::launch_gemm32(prec, f1, s), "w2v2 ffn 1");
            Gemm32Args f2{};
            f2.x = hid; f2.w_img = d.w2_img; f2.bias = d.b2; f2.residual = X; f2.out32 = P; f2.M = M; f2.N = H; f2.K = F;
            LAUNCH_OK(ppg::launch_gemm32(prec, f2, s), "w2v2 ffn 2");
            LAUNCH_OK(layer_norm(d.g2, d.e2), "w2v2 LayerNorm 2");
            continue;
        }
        {
            LinearArgs a = general(ao, H, d.wo, d.bo, H);
            a.residual = X; a.out32 = P;
            LAUNCH_OK(ppg::launch_linear(prec, EPI_GENERAL, 16, nt, a, H / 256, s), "w2v2 out-proj");
            LAUNCH_OK(layer_norm(d.g1, d.e1), "w2v2 LayerNorm 1");
        }
        {
            LinearArgs a = general(act_x, H, d.w1, d.b1, F);
            a.act_fn = 2; a.out_ld32 = F;
            if (op_copy) { a.out_rows = hid; a.out_ld = F; } else { a.out32 = reinterpret_cast<float*>(hid); }
            LAUNCH_OK(ppg::launch_linear(prec, EPI_GENERAL, 16, nt, a, F / 256, s), "w2v2 ffn 1");
            LinearArgs b = general(hid, F, d.w2, d.b2, H);
            b.residual = X; b.out32 = P;
            LAUNCH_OK(ppg::launch_linear(prec, EPI_GENERAL, 16, nt, b, H / 256, s), "w2v2 ffn 2");
            LAUNCH_OK(layer_norm(d.g2, d.e2), "w2v2 LayerNorm 2");
        }
    }
    HIP_OK(hipMemcpy2DAsync(out, (size_t)frames * H * 4, X, (size_t)R * H * 4, (size_t)frames * H * 4, batch, hipMemcpyDeviceToDevice, s));
    return PPG_OK;
}
}  // namespace

int ppg_w2v2_body_workspace_bytes(const PpgW2v2Body* body, int batch, int frames, size_t* bytes) {
    if (!body || !bytes || batch <= 0 || frames <= 0) return fail(PPG_EINVAL, "bad argument");
    const int h = body_first_half(body, batch, frames);
    *bytes = h ? align_up(body_layout(body, h, frames).total, 256) + body_layout(body, batch - h, frames).total
               : body_layout(body, batch, frames).total;
    return PPG_OK;
}

int ppg_w2v2_body_forward(PpgW2v2Body* m, const float* features, const int64_t* valid_frames, int batch, int frames,
                          float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || !features || !valid_frames || !out || !workspace || batch <= 0 || frames <= 0) return fail(PPG_EINVAL, "bad argument");
    for (int b = 0; b < batch; ++b)
        if (valid_frames[b] < 1 || valid_frames[b] > frames) return fail(PPG_EINVAL, "valid_frames[%d]=%lld outside [1, %d]", b, (long long)valid_frames[b], frames);
    size_t need = 0;
    (void)ppg_w2v2_body_workspace_bytes(m, batch, frames, &need);
    if (workspace_bytes < need) return fail(PPG_EWORKSPACE, "workspace %zu bytes < required %zu", workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 256) return fail(PPG_EINVAL, "workspace not 256-byte aligned");
    HIP_OK(hipSetDevice(m->pack.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int h = body_first_half(m, batch, frames);
    if (!h) return body_forward_one(m, m->slot[0], features, valid_frames, batch, frames, out, workspace, workspace_bytes, s);
    const size_t ws0 = align_up(body_layout(m, h, frames).total, 256);
    return fork_join(s, m->ev_fork, &m->side, &m->ev_join, 1, [&]() -> int {
        const int rc = body_forward_one(m, m->slot[1], features + (size_t)h * frames * 512, valid_frames + h, batch - h, frames,
                                        out + (size_t)h * frames * m->hidden, static_cast<char*>(workspace) + ws0, workspace_bytes - ws0, m->side);
        if (rc) return rc;
        return body_forward_one(m, m->slot[0], features, valid_frames, h, frames, out, workspace, ws0, s);
    });
}

}  // extern "C"
