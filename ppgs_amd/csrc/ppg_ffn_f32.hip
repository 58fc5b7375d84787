// The fused FFN kernels (ppg_ffn.h) in fp32.
#include "ppg_ffn.h"

template hipError_t ppg::launch_ffn_p<PrecF32>(const FfnArgs&, int, hipStream_t);
