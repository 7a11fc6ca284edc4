// rt_packet_area.hip — the packet kernel's area-light variants (rt_packet_kernel.hpp), in their
// own translation unit so that they are scheduled with the compiler's default strategy (C5 -2 %
// against max-ilp, which the other variants keep: rt_packet.hip).
#include "rt_packet_kernel.hpp"

#pragma clang fp contract(off)

namespace rtamd {

hipError_t launch_packet_area(const TraceParams& p, bool count, size_t lds, int chunks,
                              hipStream_t stream) {
    if (p.np == 0 && p.nl == 0 && chunks <= 1)
        launch_packet_variant<1, kFeatArea | kFeatNoPL>(p, count, lds, stream);
    else if (chunks <= 1) launch_packet_variant<1, kFeatArea>(p, count, lds, stream);
    else if (chunks <= 4) launch_packet_variant<4, kFeatArea>(p, count, lds, stream);
    else launch_packet_variant<16, kFeatArea>(p, count, lds, stream);
    return hipGetLastError();
}

}  // namespace rtamd
