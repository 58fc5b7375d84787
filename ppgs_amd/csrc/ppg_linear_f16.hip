// The linear / conv kernels (ppg_linear.h) in fp16.
#include "ppg_linear.h"

template hipError_t ppg::launch_linear_p<PrecF16>(int, int, int, const LinearArgs&, int, hipStream_t);
