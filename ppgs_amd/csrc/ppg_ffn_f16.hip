// The fused FFN kernels (ppg_ffn.h) in fp16, the mixed tiling among them.
#include "ppg_ffn.h"

template hipError_t ppg::launch_ffn_p<PrecF16>(const FfnArgs&, int, hipStream_t);
