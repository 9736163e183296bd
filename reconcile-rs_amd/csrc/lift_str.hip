// lift_str.hip -- the short-string-key lift (lift_str.hpp) instantiated for the three row widths, and
// its launcher.
#include "internal.hpp"
#include "lift_str.hpp"

namespace rh {

namespace {

template <int W, int RK, bool TAGS>
hipError_t launch_str(const VarCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums, hipStream_t st) {
    const uint64_t waves = (n + STR_PER_WAVE - 1) / STR_PER_WAVE;
    // multi-chunk messages first: the short kernel's block sums read their fingerprints
    hipLaunchKernelGGL((k_lift_str_long<W, RK, TAGS>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, c, n, fps);
    hipLaunchKernelGGL((k_lift_str_short<W, RK, TAGS>), dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, st, c, n, fps,
                       c.dst ? nullptr : bsums);
    return hipGetLastError();
}

template <int W>
hipError_t launch_str_width(int rk, bool tags, const VarCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums,
                            hipStream_t st) {
    switch (rk) {
    case REC_PLAIN: return launch_str<W, REC_PLAIN, false>(c, n, fps, bsums, st);
    case REC_DATED:
        return tags ? launch_str<W, REC_DATED, true>(c, n, fps, bsums, st)
                    : launch_str<W, REC_DATED, false>(c, n, fps, bsums, st);
    case REC_PROJECTION:
        return tags ? launch_str<W, REC_PROJECTION, true>(c, n, fps, bsums, st)
                    : launch_str<W, REC_PROJECTION, false>(c, n, fps, bsums, st);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

bool str_key_supported(int w) { return w == 16 || w == 32 || w == 64; }

hipError_t launch_lift_str(int w, int rk, bool tags, const VarCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums,
                           hipStream_t st, bool *supported) {
    *supported = str_key_supported(w);
    if (!*supported || n == 0) return hipSuccess;
    return w == 16   ? launch_str_width<16>(rk, tags, c, n, fps, bsums, st)
           : w == 32 ? launch_str_width<32>(rk, tags, c, n, fps, bsums, st)
                     : launch_str_width<64>(rk, tags, c, n, fps, bsums, st);
}

}  // namespace rh
