// The host side of the dense float64 cell kernels under AddressSanitizer + UndefinedBehaviorSanitizer: mmw_diag_cells64_plan over a
// sweep of planes (cells64_plan / cells64_mixed_plan of mmw_cells64_mixed.h) and the argument and route validation of
// mmw_rd_cells64_at up to its first device call.  Built like host_sanitize.cpp: the library's translation units compiled
// host-only (hipcc --cuda-host-only -fsanitize=address,undefined: kernels become launch stubs) and linked with this driver.
// Build and run: make -C tests/cpp cells64_plan_sanitize (tests/cpp/Makefile).  Without a device nothing here touches one.
#include <cstdio>
#include <cstring>

#include "../../include/mmwgpu.h"

static int fails = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                         \
        }                                                                    \
    } while (0)

int main() {
    std::printf("%s abi %d\n", mmw_version(), mmw_abi_version());
    CHECK(mmw_abi_version() == 7 && MMW_CELLS64_DENSE == 0 && MMW_CELLS64_DIRECT == 1 && MMW_CELLS64_DENSE_MIXED == 2);
    int plan[8];
    long planned = 0, mixed = 0;
    const int chirps[] = {1, 2, 5, 8, 10, 11, 15, 30, 32, 40, 50, 56, 64, 70, 80, 100, 115, 126, 127, 128, 130, 256, 320, 65536};
    const int samples[] = {1, 2, 7, 8, 63, 64, 100, 127, 200, 254, 256, 512, 829, 830, 4096, 8000, 9000, 65535, 65536, 1 << 30};
    for (int C : chirps)
        for (int S : samples) {
            std::memset(plan, 0x5a, sizeof plan);
            CHECK(mmw_diag_cells64_plan(S, C, plan) == MMW_OK);
            CHECK(plan[0] >= 0 && plan[0] <= 2 && (plan[7] == 0 || plan[7] == 1));
            if (plan[0] == 0) {
                for (int i = 1; i < 7; ++i) CHECK(plan[i] == 0);
            } else {
                CHECK(plan[1] * plan[2] == C && plan[3] > 0 && plan[3] % 8 == 0 && plan[3] * plan[2] <= 512);
                CHECK(plan[4] > 0 && plan[4] <= 160 * 1024 - 512 && plan[5] == 256 && plan[6] > C && plan[6] % 2 == 1);
                CHECK((plan[0] == 1) == (C == 128));
                // the spectra of a pass and the plane's tables fit what the plan reports
                CHECK((long)plan[3] * plan[6] * 16 + (long)S * 16 + ((long)S + C) * 8 <= plan[4]);
            }
            if (plan[0] == 2) {
                CHECK(plan[7] == 1 && plan[1] <= 10 && plan[2] >= 2);
                ++mixed;
            }
            ++planned;
        }
    CHECK(mixed > 0);
    CHECK(mmw_diag_cells64_plan(829, 128, plan) == MMW_OK && plan[0] == 1);
    CHECK(mmw_diag_cells64_plan(830, 128, plan) == MMW_OK && plan[0] == 0 && plan[7] == 1);
    CHECK(mmw_diag_cells64_plan(63, 100, plan) == MMW_OK && plan[0] == 2 && plan[1] == 10 && plan[2] == 10 && plan[3] == 48);
    CHECK(mmw_diag_cells64_plan(63, 127, plan) == MMW_OK && plan[0] == 0 && plan[7] == 0);
    CHECK(mmw_diag_cells64_plan(0, 100, plan) == MMW_ERR_INVALID && std::strlen(mmw_last_error()) > 0);
    CHECK(mmw_diag_cells64_plan(63, -1, plan) == MMW_ERR_INVALID);
    CHECK(mmw_diag_cells64_plan(63, 100, nullptr) == MMW_ERR_INVALID);

    // mmw_rd_cells64_at: everything it rejects before a device is needed.  No context can exist on a machine without a GPU, so
    // the null-context check comes first; with a context (where a device exists) the shape, route and antenna-list checks run
    // before the first copy.
    int ants[4] = {0, 1, 2, 3};
    char dummy[64] = {0};
    for (int route = -1; route <= 3; ++route)
        CHECK(mmw_rd_cells64_at(nullptr, dummy, (const int32_t *)dummy, (const int32_t *)dummy, dummy, 1, 4, 63, 100, 1, ants, 4, route) == MMW_ERR_INVALID);
    mmw_ctx *ctx = nullptr;
    if (mmw_ctx_create(&ctx, 0) == MMW_OK && ctx) {
        const int32_t *d = (const int32_t *)dummy;
        CHECK(mmw_rd_cells64_at(ctx, nullptr, d, d, dummy, 1, 4, 63, 100, 1, ants, 4, 2) == MMW_ERR_INVALID);
        CHECK(mmw_rd_cells64_at(ctx, dummy, d, d, dummy, 1, 4, 63, 100, 1, ants, 4, 3) == MMW_ERR_INVALID);         // no such route
        CHECK(mmw_rd_cells64_at(ctx, dummy, d, d, dummy, 1, 4, 63, 100, 1, ants, 4, -1) == MMW_ERR_INVALID);
        CHECK(mmw_rd_cells64_at(ctx, dummy, d, d, dummy, 1, 4, 65536, 100, 1, ants, 4, 2) == MMW_ERR_INVALID);      // S beyond the cell packing
        CHECK(mmw_rd_cells64_at(ctx, dummy, d, d, dummy, 70000, 4, 63, 100, 1, ants, 4, 2) == MMW_ERR_INVALID);
        CHECK(mmw_rd_cells64_at(ctx, dummy, d, d, dummy, 1, 4, 63, 100, 1, ants, 0, 2) == MMW_ERR_INVALID);         // empty antenna list
        ants[3] = 4;
        CHECK(mmw_rd_cells64_at(ctx, dummy, d, d, dummy, 1, 4, 63, 100, 1, ants, 4, 2) == MMW_ERR_INVALID);         // antenna 4 of 4
        ants[3] = 3;
        CHECK(mmw_rd_cells64_at(ctx, dummy, d, d, dummy, 1, 4, 16, 320, 1, ants, 4, 2) == MMW_ERR_UNSUPPORTED);     // no instantiation
        CHECK(mmw_rd_cells64_at(ctx, dummy, d, d, dummy, 1, 4, 63, 100, 1, ants, 4, 0) == MMW_ERR_UNSUPPORTED);     // route 0: 128 chirps only
        CHECK(mmw_rd_cells64_at(ctx, dummy, d, d, dummy, 1, 4, 9000, 100, 1, ants, 4, 2) == MMW_ERR_UNSUPPORTED);   // tables beyond the LDS
        CHECK(mmw_rd_cells64_at(ctx, dummy, d, d, dummy, 0, 4, 63, 100, 1, ants, 4, 2) == MMW_OK);                  // nothing to do
        mmw_ctx_destroy(ctx);
    } else {
        std::printf("no device: the context-dependent checks of mmw_rd_cells64_at are skipped (%s)\n", mmw_last_error());
    }
    std::printf("%ld planes planned, %ld with the mixed kernel, %d failures\n", planned, mixed, fails);
    return fails ? 1 : 0;
}
