// The wave-specialised convolution kernel (conv_ws.h): its one-plane (bf16) and two-plane forward instantiations, and the launcher
// of the family.  The two-plane data gradients are instantiated in conv_ws_dgrad.hip.
#define CONV_WS_PLANES_MODE 0
#include "conv_ws.h"

namespace {

template <typename T, int MODE>
void launch_ws(const cc::ConvChoice& c, const ConvArgs& a, hipStream_t st) {
    const dim3 grid(c.grid), block(c.block);
    if constexpr (sizeof(T) == 2) {
        if (c.mw == 1)
            hipLaunchKernelGGL((conv_ws_kernel<1, 4, MODE, cc::WS_NLD>), grid, block, 0, st, a, c.kx_bytes, c.kw_bytes);
        else
            hipLaunchKernelGGL((conv_ws_kernel<2, 2, MODE, cc::WS_NLD>), grid, block, 0, st, a, c.kx_bytes, c.kw_bytes);
    } else if constexpr (MODE == 1) {
        launch_conv_ws_dgrad_planes(c, a, st);
    } else if constexpr (MODE == 0) {
        launch_ws_planes<0, 0>(c, a, st);
    }
}

}  // namespace

void conv_device::launch_conv_ws(const cc::ConvChoice& c, const ConvArgs& a, hipStream_t st) {
    if (c.elem_bytes == 2) {
        if (c.mode == 2) launch_ws<bf16_t, 2>(c, a, st);
        else if (c.mode == 1) launch_ws<bf16_t, 1>(c, a, st);
        else launch_ws<bf16_t, 0>(c, a, st);
    } else {
        if (c.mode == 1) launch_ws<float, 1>(c, a, st);
        else launch_ws<float, 0>(c, a, st);
    }
}
