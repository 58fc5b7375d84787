// The linear / conv kernels (ppg_linear.h) on split-precision operands (fp16x2).
#include "ppg_linear.h"

template hipError_t ppg::launch_linear_p<PrecX2>(int, int, int, const LinearArgs&, int, hipStream_t);
