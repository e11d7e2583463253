// The wave-specialised convolution kernel (conv_ws.h): its two-plane data-gradient instantiations, reached through conv_ws.hip.
#define CONV_WS_PLANES_MODE 1
#include "conv_ws.h"

void conv_device::launch_conv_ws_dgrad_planes(const cc::ConvChoice& c, const ConvArgs& a, hipStream_t st) {
    // data gradients: one instantiation per set of epilogue operands (conv_epilogue_rows_ops)
    if (c.epi == 3) launch_ws_planes<1, 3>(c, a, st);
    else if (c.epi == 2) launch_ws_planes<1, 2>(c, a, st);
    else if (c.epi == 1) launch_ws_planes<1, 1>(c, a, st);
    else launch_ws_planes<1, 0>(c, a, st);
}
