// The linear / conv kernels (ppg_linear.h) in bf16.
#include "ppg_linear.h"

template hipError_t ppg::launch_linear_p<PrecBF16>(int, int, int, const LinearArgs&, int, hipStream_t);
