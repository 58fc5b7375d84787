// ppg::launch_linear: dispatch on the precision.  The kernels and the choice of an instantiation are ppg_linear.h,
// compiled once per precision in ppg_linear_<precision>.hip; this unit sees only the declaration, so it holds no kernel.
#include "ppg_device.h"
#include "ppg_launch.h"

namespace ppg {

template <class P>
hipError_t launch_linear_p(int epi, int nb, int nt, const LinearArgs& a, int ypasses, hipStream_t s);
extern template hipError_t launch_linear_p<PrecBF16>(int, int, int, const LinearArgs&, int, hipStream_t);
extern template hipError_t launch_linear_p<PrecX2>(int, int, int, const LinearArgs&, int, hipStream_t);
extern template hipError_t launch_linear_p<PrecF16>(int, int, int, const LinearArgs&, int, hipStream_t);
extern template hipError_t launch_linear_p<PrecF32>(int, int, int, const LinearArgs&, int, hipStream_t);

hipError_t launch_linear(int precision, int epi, int nb, int nt, const LinearArgs& a, int ypasses, hipStream_t s) {
    if (precision == PPG_PRECISION_BF16) return launch_linear_p<PrecBF16>(epi, nb, nt, a, ypasses, s);
#if PPG_X2
    if (precision == PPG_PRECISION_FP16X2) return launch_linear_p<PrecX2>(epi, nb, nt, a, ypasses, s);
#endif
#if PPG_OTHER_PRECISIONS
    if (precision == PPG_PRECISION_FP16) return launch_linear_p<PrecF16>(epi, nb, nt, a, ypasses, s);
    return launch_linear_p<PrecF32>(epi, nb, nt, a, ypasses, s);
#else
    return hipErrorInvalidValue;
#endif
}

}  // namespace ppg
