// mmw_lsq_core.h's bands, adjugate solve and R^2 on the host, as a program of its own (no device, no library): it reads one request
// per line from standard input -- a name and its arguments, floating-point values as C hex floats -- and prints the results as hex
// floats, so tests/test_lsq_band_cases_host.py can hold the Python restatement of the bands against the code the kernels run.
// Built with -ffp-contract=off, as every unit that includes the header must be.
//
//   coef n cond scale                 -> lsq_band_coef
//   residual band_c ymax c1           -> lsq_band_residual (unit rows: hmax = 1)
//   sq r band_r                       -> lsq_band_sq
//   sumsq m band_r sr sr2             -> lsq_band_sum_sq
//   r2 m ymax band_r sr2 sr syy       -> lsq_r2_of_sums: value, band, loose
//   solve dim g[6] b[3]               -> lsq_gram_solve: c[3], cond
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../mmwave_radar_processing_amd/csrc/mmw_lsq_core.h"

int main() {
    char line[1024];
    int served = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        char name[16] = {0};
        double v[10] = {0};
        int n = 0, used = 0;
        if (std::sscanf(line, "%15s%n", name, &used) != 1) continue;
        for (char *p = line + used, *end = nullptr; n < 10; p = end, ++n) {
            v[n] = std::strtod(p, &end);
            if (end == p) break;
        }
        if (!std::strcmp(name, "coef") && n == 3) {
            std::printf("%a\n", mmw::lsq_band_coef((int)v[0], v[1], v[2]));
        } else if (!std::strcmp(name, "residual") && n == 3) {
            std::printf("%a\n", mmw::lsq_band_residual(v[0], 1.0, v[1], v[2]));
        } else if (!std::strcmp(name, "sq") && n == 2) {
            std::printf("%a\n", mmw::lsq_band_sq(v[0], v[1]));
        } else if (!std::strcmp(name, "sumsq") && n == 4) {
            std::printf("%a\n", mmw::lsq_band_sum_sq((int)v[0], v[1], v[2], v[3]));
        } else if (!std::strcmp(name, "r2") && n == 6) {
            double band;
            bool loose;
            const double r2 = mmw::lsq_r2_of_sums((int)v[0], v[1], v[2], v[3], v[4], v[5], &band, &loose);
            std::printf("%a %a %d\n", r2, band, loose ? 1 : 0);
        } else if (!std::strcmp(name, "solve") && n == 10) {
            double c[3], cond;
            mmw::lsq_gram_solve((int)v[0], v + 1, v + 7, c, &cond);
            std::printf("%a %a %a %a\n", c[0], c[1], c[2], cond);
        } else {
            std::fprintf(stderr, "lsq_core_bands: bad request: %s", line);
            return 2;
        }
        ++served;
    }
    std::fprintf(stderr, "lsq_core_bands: %d requests\n", served);
    return 0;
}
