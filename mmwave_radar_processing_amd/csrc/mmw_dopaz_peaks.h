// Peak picking on batched Doppler-azimuth maps (mmw_doppler_azimuth_peaks): what
// DopplerAzimuthProcessor.detect_peaks_rows / detect_peak_zero_az decide in dB with scipy.signal.find_peaks, decided in the linear
// domain in float64 (every decision of the pickers is monotone in the linear value, and no log10 is evaluated here).
//
//   dzp_value / dzp_pick   the rule, ONE __host__ __device__ implementation: the kernel and the host-only entry
//                          mmw_diag_doppler_azimuth_peaks_host both call it, line by line.
//   k_dopaz_peaks          one workgroup per (group, frame): phase 1 widens the frame's valid cells to y = |avg| + 1e-12, keeps them
//                          in the LDS (DZP_LS doubles per row) and reduces the frame maximum and a non-finite flag; phase 2 gives
//                          every line -- the m rows and the zero-azimuth column -- to one thread, which runs dzp_pick on it.
//
// A comparison whose operands lie inside the relative band MMW_DOPAZ_PEAK_BAND is not decided here: the line becomes
// DZP_UNDECIDED and the host picks that frame again with the dB rule.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "../../include/mmwgpu.h"
#include "mmw_dopaz_codes.h"             // DZP_NONE, DZP_UNDECIDED

namespace mmw {

constexpr int DZP_LS = 65;              // doubles per row of the LDS image: an odd stride, so that the 64 threads of a wave, each
                                        // walking a row of its own, read 32 distinct banks per half wave (ds_read_b64)
constexpr int DZP_LDS_HEAD = 64;        // bytes in front of the image: four wave maxima, four non-finite flags
constexpr size_t DZP_LDS_MAX = 160 * 1024;

struct DzpRule {
    double fl;              // the floor: frame maximum * floor_ratio
    double prom;            // 10^(prominence_dB / 20)
    bool fl_exact;          // floor_ratio == 1: fl IS the frame maximum, so a cell bit-equal to it is decided (floored)
    bool prom_exact;        // prom == 1
};

// y of cell i of one map, or of two maps averaged as the reference's (resp_1 + resp_2) / 2 on float64: the IEEE operations numpy
// performs on the widened float32 values, so y is bit-identical to the host's abs(map) + 1e-12
__host__ __device__ inline double dzp_value(const float *m1, const float *m2, long i) {
    const double v = m2 ? ((double)m1[i] + (double)m2[i]) / 2.0 : (double)m1[i];
    return fabs(v) + 1e-12;
}

// Two map-derived quantities the host compares through their dB values: decided when bit-equal or further apart than the band.
__host__ __device__ inline bool dzp_close(double a, double b) { return a != b && fabs(a - b) <= MMW_DOPAZ_PEAK_BAND * fmax(a, b); }

// A map-derived quantity against a product with a ratio (the floor, base * prominence): the product carries a rounding of its
// own, so even bit-equal operands say nothing about the host's dB comparison -- unless the ratio is exactly 1.
__host__ __device__ inline bool dzp_close_product(double a, double prod, bool exact) {
    return fabs(a - prod) <= MMW_DOPAZ_PEAK_BAND * fmax(a, prod) && !(exact && a == prod);
}

struct DzpLine {            // a line of y kept in memory
    const double *p;
    int stride;
    __host__ __device__ double operator()(int i) const { return p[(long)i * stride]; }
};

struct DzpMapLine {         // a line of y made from the maps on every access (frames whose image does not fit the LDS)
    const float *m1, *m2;
    long stride;
    __host__ __device__ double operator()(int i) const { return dzp_value(m1, m2, i * stride); }
};

// The choice on one line of n values y(0) .. y(n - 1): the index of the strongest local maximum (with prominence: of those whose
// value reaches base * R.prom), DZP_NONE, or DZP_UNDECIDED.
//   floor       y <= R.fl becomes R.fl (that is what makes the plateaus)
//   maxima      scipy's _local_maxima_1d: a run of equal values strictly above both neighbours is one peak at (first + last) / 2;
//               the first and the last sample are never peaks
//   prominence  scipy's peak_prominences, wlen=None: from the peak to each side while values are <= the peak, the minimum of each
//               side; base = the larger minimum
//   choice      the largest value, the first of equals (np.argmax)
template <class Line>
__host__ __device__ inline int dzp_pick(const Line &y, int n, const DzpRule &R, bool prominence) {
    if (n < 3) return DZP_NONE;
    auto f = [&](int i) {
        const double v = y(i);
        return v <= R.fl ? R.fl : v;
    };
    // the floor test of every cell and every pair of neighbours, before anything is decided
    double prev = 0.0;
    for (int i = 0; i < n; ++i) {
        const double v = y(i);
        if (dzp_close_product(v, R.fl, R.fl_exact)) return DZP_UNDECIDED;
        const double fv = v <= R.fl ? R.fl : v;
        if (i > 0 && dzp_close(prev, fv)) return DZP_UNDECIDED;
        prev = fv;
    }
    int best = DZP_NONE;
    double best_v = 0.0;
    bool rival = false;         // a candidate inside the band of the best one, not bit-equal to it
    const int i_max = n - 1;
    for (int i = 1; i < i_max; ++i) {
        const double v = f(i);
        if (!(f(i - 1) < v)) continue;
        int ahead = i + 1;
        while (ahead < i_max && f(ahead) == v) ++ahead;
        if (!(f(ahead) < v)) continue;
        const int p = (i + ahead - 1) / 2;
        i = ahead;
        if (prominence) {
            double lmin = v, rmin = v;
            for (int j = p; j >= 0; --j) {
                const double w = f(j);
                if (w > v) {
                    if (dzp_close(w, v)) return DZP_UNDECIDED;
                    break;
                }
                lmin = fmin(lmin, w);
            }
            for (int j = p; j < n; ++j) {
                const double w = f(j);
                if (w > v) {
                    if (dzp_close(w, v)) return DZP_UNDECIDED;
                    break;
                }
                rmin = fmin(rmin, w);
            }
            const double need = fmax(lmin, rmin) * R.prom;
            if (dzp_close_product(v, need, R.prom_exact)) return DZP_UNDECIDED;
            if (!(v >= need)) continue;
        }
        if (best < 0 || v > best_v) {
            rival = best >= 0 && dzp_close(v, best_v);
            best = p;
            best_v = v;
        } else if (dzp_close(v, best_v)) {
            rival = true;
        }
    }
    return rival ? DZP_UNDECIDED : best;
}

struct DzpArgs {
    const float *maps;          // [n_sets][F][n_rows][64]
    long set_stride;            // F * n_rows * 64
    const int2 *groups;         // [G]: two sets averaged, or (set, -1)
    const int *m;               // [F] rows of each frame, or null: n_rows
    int F, n_rows, a_lo, a_hi, a_zero;
    double floor_ratio;         // 10^(-min_threshold_dB / 20)
    DzpRule rule;               // fl is filled in per frame
    int *row_peak;              // [G][F][n_rows]
    int *zero;                  // [G][F]
};

inline size_t dopaz_peaks_lds(int rows) { return DZP_LDS_HEAD + (size_t)rows * DZP_LS * sizeof(double); }

// grid (G * F), 256 threads, dopaz_peaks_lds(max m) bytes of dynamic LDS (IMAGE) or DZP_LDS_HEAD bytes (the lines are then made
// from the maps on every access).  Every output entry of the (group, frame) is written, by plain vector stores.
template <bool IMAGE>
__global__ __launch_bounds__(256) void k_dopaz_peaks(DzpArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dzp_smem[];
    double *wave_max = reinterpret_cast<double *>(dzp_smem);
    int *wave_bad = reinterpret_cast<int *>(dzp_smem + 32);
    double *img = reinterpret_cast<double *>(dzp_smem + DZP_LDS_HEAD);
    const int g = blockIdx.x / a.F, f = blockIdx.x - g * a.F;
    const int2 grp = a.groups[g];
    const int m = a.m ? a.m[f] : a.n_rows;
    const long frame = (long)f * a.n_rows * 64;
    const float *m1 = a.maps + grp.x * a.set_stride + frame;
    const float *m2 = grp.y >= 0 ? a.maps + grp.y * a.set_stride + frame : nullptr;
    const int nc = a.a_hi - a.a_lo;
    // phase 1: the frame's valid cells, their maximum, and whether one of them is not finite
    double mx = 0.0;
    bool bad = false;
    for (int i = threadIdx.x; i < m * 64; i += 256) {
        const int r = i >> 6, c = (i & 63) - a.a_lo;
        if (c < 0 || c >= nc) continue;
        const double v = dzp_value(m1, m2, i);
        bad |= !(v <= DBL_MAX);
        mx = fmax(mx, v);
        if (IMAGE) img[r * DZP_LS + c] = v;
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
    const bool wave_has_bad = __ballot(bad) != 0;
    if ((threadIdx.x & 63) == 0) {
        wave_max[threadIdx.x >> 6] = mx;
        wave_bad[threadIdx.x >> 6] = wave_has_bad;
    }
    __syncthreads();
    mx = fmax(fmax(wave_max[0], wave_max[1]), fmax(wave_max[2], wave_max[3]));
    bad = (wave_bad[0] | wave_bad[1] | wave_bad[2] | wave_bad[3]) != 0;
    DzpRule R = a.rule;
    R.fl = mx * a.floor_ratio;
    // phase 2: line L < n_rows is row L, line n_rows is the zero-azimuth column
    const long gf = (long)g * a.F + f;
    for (int L = threadIdx.x; L <= a.n_rows; L += 256) {
        const bool row = L < a.n_rows;
        int res;
        if (row && L >= m) res = DZP_NONE;
        else if (bad) res = DZP_UNDECIDED;
        else if (row)
            res = IMAGE ? dzp_pick(DzpLine{img + L * DZP_LS, 1}, nc, R, true)
                        : dzp_pick(DzpMapLine{m1 + (long)L * 64 + a.a_lo, m2 ? m2 + (long)L * 64 + a.a_lo : nullptr, 1}, nc, R, true);
        else
            res = IMAGE ? dzp_pick(DzpLine{img + (a.a_zero - a.a_lo), DZP_LS}, m, R, false)
                        : dzp_pick(DzpMapLine{m1 + a.a_zero, m2 ? m2 + a.a_zero : nullptr, 64}, m, R, false);
        if (row) a.row_peak[gf * a.n_rows + L] = res;
        else a.zero[gf] = res;
    }
}

}  // namespace mmw
