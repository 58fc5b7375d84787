// Timing builds only (-DPPG_FFN_TIMING / PPG_ATTN_TIMING / PPG_H32_TIMING / PPG_LIN_TIMING): what the stamp buffers of
// the engine's layer-0 launches hold when the engine is destroyed, printed to stderr or written to the *_TIMING_OUT file.
#include "ppg_host.h"

#ifdef PPG_TIMING_BUILD
namespace ppg {

void dump_timing_stamps(const PpgEngine* e) {
    const bool layer32 = e->layer32, split = e->split();
    unsigned long long *head_dbg = e->head_dbg, *ffn_dbg = e->ffn_dbg, *attn_dbg = e->attn_dbg, *lin_dbg = e->lin_dbg;
    if (head_dbg) {
        unsigned long long h[64];
        (void)hipDeviceSynchronize();
        if (hipMemcpy(h, head_dbg, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess)
            for (int w = 0; w < 4; ++w) {
                const unsigned long long* t = h + w * 16;
                fprintf(stderr, "head32 wave %d: gather %llu  bias+meta %llu  conv0 %llu  conv1 %llu  emit %llu  wq %llu  tail %llu | total %llu\n",
                        w, t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4], t[6] - t[5], t[7] - t[6], t[7] - t[0]);
            }
    }
    if (ffn_dbg) {
        unsigned long long h[256];
        (void)hipDeviceSynchronize();
        if (hipMemcpy(h, ffn_dbg, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess) {
            for (int i = 0; i < 6; ++i) {
                const unsigned long long* t = h + 192 + i * 8;
                if (t[0]) fprintf(stderr, "ffn qkv tail tile %d: wait %llu barrier %llu mfma %llu stores %llu dma %llu | total %llu\n", i + 4,
                                  t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4], t[5] - t[0]);
            }
            for (int w = 0; w < 4; ++w) {
                const unsigned long long* t = h + 128 + w * 16;
                fprintf(stderr, "ffn prologue wave %d:", w);
                for (int k = 1; k < 15; ++k) if (t[k]) fprintf(stderr, " [%d] %llu", k, t[k] - t[0]);
                fprintf(stderr, "\n");
            }
            if (layer32 || split) {
                for (int w = 0; w < 4; ++w) {
                    const unsigned long long* t = h + w * 8;
                    if (split)
                        fprintf(stderr, "ffn32x2 wave %d chunk 4: A1 %llu  wait %llu  A2 %llu  hand-over + barrier + wait %llu  B1 %llu  B2 (+ wait) %llu | total %llu\n",
                                w, t[1] - t[0], t[6] - t[1], t[7] - t[6], t[2] - t[7], t[3] - t[2], t[5] - t[3], t[5] - t[0]);
                    else
                    fprintf(stderr, "layer32 wave %d chunk 4 (hidden 256: one stream): A blocks 0-2 %llu  A blocks 3,4 + h writes %llu  B blocks 0-2 + h writes %llu  B blocks 3,4 %llu | total %llu\n",
                            w, t[1] - t[0], t[2] - t[1], t[3] - t[2], t[5] - t[3], t[5] - t[0]);
                }
            } else
            for (int w = 0; w < 4; ++w)
                for (int c = 0; c < 4; ++c) {
                    const unsigned long long* t = h + (w * 4 + c) * 8;
                    fprintf(stderr, "ffn timing wave %d chunk %d: dma-issue %llu  A+pack %llu  B %llu  vmcnt %llu  barrier %llu | total %llu\n",
                            w, c + 8, t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4], t[5] - t[0]);
                }
        }
    }
    if (attn_dbg) {
        unsigned long long h[64];
        (void)hipDeviceSynchronize();
        if (hipMemcpy(h, attn_dbg, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess)
            for (int w = 0; w < 4; ++w)
                for (int c = 0; c < 2; ++c) {
                    const unsigned long long* t = h + (w * 2 + c) * 8;
                    fprintf(stderr, "attn timing wave %d tile %d: dma-issue %llu  scores+softmax %llu  PV %llu  vmcnt %llu  barrier %llu | total %llu\n",
                            w, c + 2, t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4], t[5] - t[0]);
                }
        {   // per-workgroup records: start, end, valid keys, HW_ID -> PPGS_AMD_ATTN_TIMING_OUT (tools/attn_timeline.py)
            std::vector<unsigned long long> rec(4096 * 4);
            const char* path = getenv("PPGS_AMD_ATTN_TIMING_OUT");   // (PPG_ATTN_TIMING builds only: attn_dbg is null otherwise)
            if (path && hipMemcpy(rec.data(), attn_dbg + 64, rec.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
                FILE* f = fopen(path, "wb");
                if (f) { fwrite(rec.data(), 8, rec.size(), f); fclose(f); }
            }
        }
    }
    if (lin_dbg) {
        const size_t n = 16 * 8192;
        std::vector<unsigned long long> h(n);
        (void)hipDeviceSynchronize();
        const char* path = getenv("PPGS_AMD_LIN_TIMING_OUT");   // (PPG_LIN_TIMING builds only)
        FILE* f = fopen(path ? path : "/tmp/lin_timing.bin", "wb");
        if (f && hipMemcpy(h.data(), lin_dbg, n * 8, hipMemcpyDeviceToHost) == hipSuccess) fwrite(h.data(), 8, n, f);
        if (f) fclose(f);
    }
}

}  // namespace ppg
#endif
