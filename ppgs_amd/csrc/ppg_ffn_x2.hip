// The fused FFN kernels (ppg_ffn.h) on split-precision operands (fp16x2): hidden 256, unfused.
#include "ppg_ffn.h"

template hipError_t ppg::launch_ffn_p<PrecX2>(const FfnArgs&, int, hipStream_t);
