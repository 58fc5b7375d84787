// ppg::launch_ffn: dispatch on the precision.  The kernels and the choice of an instantiation are ppg_ffn.h, compiled
// once per precision in ppg_ffn_<precision>.hip; this unit sees only the declaration, so it holds no kernel.
#include "ppg_device.h"
#include "ppg_launch.h"

namespace ppg {

template <class P>
hipError_t launch_ffn_p(const FfnArgs& a, int nt, hipStream_t s);
extern template hipError_t launch_ffn_p<PrecBF16>(const FfnArgs&, int, hipStream_t);
extern template hipError_t launch_ffn_p<PrecX2>(const FfnArgs&, int, hipStream_t);
extern template hipError_t launch_ffn_p<PrecF16>(const FfnArgs&, int, hipStream_t);
extern template hipError_t launch_ffn_p<PrecF32>(const FfnArgs&, int, hipStream_t);

hipError_t launch_ffn(int precision, const FfnArgs& a, int nt, hipStream_t s) {
    if (precision == PPG_PRECISION_BF16) return launch_ffn_p<PrecBF16>(a, nt, s);
#if PPG_X2
    if (precision == PPG_PRECISION_FP16X2) return launch_ffn_p<PrecX2>(a, nt, s);
#endif
#if PPG_OTHER_PRECISIONS
    if (precision == PPG_PRECISION_FP16) return launch_ffn_p<PrecF16>(a, nt, s);
    return launch_ffn_p<PrecF32>(a, nt, s);
#else
    return hipErrorInvalidValue;
#endif
}

}  // namespace ppg
