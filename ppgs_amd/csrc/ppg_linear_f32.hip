// The linear / conv kernels (ppg_linear.h) in fp32.
#include "ppg_linear.h"

template hipError_t ppg::launch_linear_p<PrecF32>(int, int, int, const LinearArgs&, int, hipStream_t);
