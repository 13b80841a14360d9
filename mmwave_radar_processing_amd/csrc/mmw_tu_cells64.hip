// Translation unit: k_cells64_mixed<C>, the dense float64 cell kernel of the chirp counts other than 128 (mmw_cells64_mixed.h).
#include "mmw_ctx.h"
#include "mmw_cells64_mixed.h"

namespace mmw {

int launch_cells64_mixed(mmw_ctx *ctx, const Cells64Args &ca, int C, int n_frames, size_t lds) {
    switch (C) {
#define X(CC)                                                                                                                  \
    case CC:                                                                                                                   \
        MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_cells64_mixed<CC>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                    (int)lds));                                                                                \
        hipLaunchKernelGGL(k_cells64_mixed<CC>, dim3((unsigned)ca.n_ant, (unsigned)n_frames), dim3(C64_NT), lds, ctx->stream, ca); \
        return check_launch("cells64_mixed");
        MMW_CELLS64_MIXED_C(X)
#undef X
    default:
        return set_error(MMW_ERR_UNSUPPORTED, "no dense float64 cell kernel for %d chirps", C);
    }
}

}  // namespace mmw
