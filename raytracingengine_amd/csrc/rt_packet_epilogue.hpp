// rt_packet_epilogue.hpp — the end of a pixel in packet_direct_kernel and packet_uniform_kernel:
// the fix-list append (kFeatFix), then the f64, f32 and byte stores of the pixel (x_e, yl_e) of
// the frame at frame_off, for the lanes that have one (lanes past the image edge have none).
// A fragment, not a header: included inside both kernels' bodies, so there is one text and each
// kernel compiles it as its own statements (as a function of its own it was optimised before
// inlining and changed the instruction selection of every instantiation).  It reads, from the
// enclosing scope: FEAT (constexpr int), P (TraceParams), lane_e, x_e, yl_e (uint32_t), frame_off
// (uint64_t), acc (d3), samples (int), fix (bool).
    bool store = x_e < P.width && yl_e < P.rows;
    if constexpr ((FEAT & kFeatFix) != 0) {
        // the pixels with an undecided shadow ray: appended to the fix-up list (one atomic per
        // wave), rendered by packet_fixup_kernel after this launch instead of stored here
        const bool q = fix && store;
        const uint64_t bq = __ballot(q);
        if (bq) {
            uint32_t base = 0;
            if (lane_e == static_cast<uint32_t>(__builtin_ctzll(bq)))
                base = atomicAdd(P.fix_ctl, static_cast<uint32_t>(__builtin_popcountll(bq)));
            base = __shfl(base, __builtin_ctzll(bq), 64);
            if (q)
                P.fix_list[base + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bq >> 32),
                                                            __builtin_amdgcn_mbcnt_lo(
                                                                static_cast<uint32_t>(bq), 0u))] =
                    static_cast<uint32_t>(frame_off + static_cast<size_t>(yl_e) * P.width + x_e);
        }
        store = store && !fix;
    }
    if (store) {
        // accumulated / samples (Scene.h:298-300); x / 1.0 == x, so AA=1 skips the division
        const d3 v = samples == 1 ? acc
                   : (samples > 0 ? sdiv(acc, static_cast<double>(samples)) : mk(0.0, 0.0, 0.0));
        const size_t o = frame_off + static_cast<size_t>(yl_e) * P.width + x_e;
        if (P.out64) {
            P.out64[3 * o + 0] = v.x;
            P.out64[3 * o + 1] = v.y;
            P.out64[3 * o + 2] = v.z;
        }
        if (P.out32) {
            P.out32[3 * o + 0] = static_cast<float>(v.x);
            P.out32[3 * o + 1] = static_cast<float>(v.y);
            P.out32[3 * o + 2] = static_cast<float>(v.z);
        }
        if (P.ldr) {
            uint8_t r, g, b;
            if (P.tonemap == 1) {  // uniform: Reinhard, through the FP32 byte decision
                r = reinhard_byte(v.x);
                g = reinhard_byte(v.y);
                b = reinhard_byte(v.z);
            } else if constexpr ((FEAT & kFeatJodie) != 0) {
                to_color(tonemap_op(v, P.tonemap), r, g, b);
            } else {
                to_color(tonemap_op_nolog(v, P.tonemap), r, g, b);
            }
            P.ldr[3 * o + 0] = r;
            P.ldr[3 * o + 1] = g;
            P.ldr[3 * o + 2] = b;
        }
    }
