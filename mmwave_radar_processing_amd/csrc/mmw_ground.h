// Batched ground detector (FramePipeline(ground=...)): the state-free parts of
// RangeDopplerGroundDetector.process for F frames at once.
//
//   k_ground_peaks      one workgroup per frame: RangeProcessor.find_peaks on the float64 chirp-0 range profile
//                       (processors/range_resp.py:104-149) -> at most 3 candidate ranges, strongest first
//   k_ground_zoom       one workgroup per (frame, coarse candidate): Altimeter._look_zoom's window around the candidate,
//                       the mean-over-antennas |DFT| of chirp 0 on S bins in float64, then the same picker (2 peaks)
//   k_cfar1d_gated      the Doppler CFAR (cfar1d_threshold, the code of k_cfar1d) on the rows near..far of each frame's
//                       float64 |RD| plane (or on a list of rows: the sequential detector's full-plane route); k_compact2d
//                       then lists the hits in row-major order
//
// The picker decides every comparison scipy makes on 20 log10(p) -- neighbours and plateaus, the prominence bases, the
// 6-dB prominence, the `>= max - 20` cut, the final ordering -- from the device's own 20 log10(p).  Device (OCML) and host
// log10 differ by a few ulps: |y_dev - y_host| <= 20 * (4 + 4) ulp(log10 p) + ulp(y) < 1e-12 dB for any finite p > 0
// (|log10 p| < 308).  Equal linear values compare equal on both sides (log10 is a function).  Any other decision whose two
// sides lie within PEAK_BAND_DB (1e-9 dB, a thousand times that bound) is UNDECIDED: the frame / window is flagged
// (count -1) and the host re-runs RangeProcessor.find_peaks on the profile / spectrum this code left in memory.
#pragma once
#include "mmw_cfar.h"

namespace mmw {

constexpr double PEAK_BAND_DB = 1e-9;
constexpr int GROUND_COARSE = 3;         // Altimeter._look_coarse: max_peaks=3
constexpr int GROUND_FINE = 2;           // Altimeter._look_zoom: max_peaks=2
constexpr int PEAK_LIST = 512;           // peaks of >= 6 dB prominence one workgroup keeps; more -> flagged
constexpr int ZOOM_VB = 16;              // antennas staged per pass of k_ground_zoom
constexpr int ZOOM_BINS_PER_THREAD = 8;  // S <= 2048

// scipy's comparison of samples a and b of x = 20 log10(p): -1, 0, 1.  Distinct values closer than the band set *und.
__device__ __forceinline__ int db_cmp(const double *p, const double *y, int a, int b, int *und) {
    if (p[a] == p[b]) return 0;
    const double d = y[a] - y[b];
    if (!(fabs(d) > PEAK_BAND_DB)) *und = 1;            // also NaN (non-finite input): the host decides
    return p[a] < p[b] ? -1 : 1;
}

// scipy.signal.find_peaks(y, prominence=6) (local maxima with the plateau midpoint, first / last sample never a peak,
// prominence with wlen=None), then `vals >= max(vals) - 20`, then argsort(vals)[::-1][:max_peaks].  p (linear) and y (dB)
// in LDS, n samples, the whole workgroup calls it.  Returns the number of peaks (indices in top[], strongest first) or -1
// when a decision is undecided.
__device__ int pick_peaks(const double *p, const double *y, int n, int max_peaks, int *list, int *n_list, int *top) {
    int und = 0;
    if (threadIdx.x == 0) *n_list = 0;
    __syncthreads();
    for (int i = 1 + (int)threadIdx.x; i < n - 1; i += (int)blockDim.x) {
        if (db_cmp(p, y, i - 1, i, &und) >= 0) continue;             // the rising edge of a peak or plateau
        int r = i + 1;
        while (r < n - 1 && db_cmp(p, y, r, i, &und) == 0) ++r;
        if (db_cmp(p, y, r, i, &und) >= 0) continue;
        const int peak = (i + r - 1) / 2;
        int lb = peak, rb = peak;                                    // lowest sample before a higher one, each side
        for (int k = peak - 1; k >= 0 && db_cmp(p, y, k, peak, &und) <= 0; --k)
            if (db_cmp(p, y, k, lb, &und) < 0) lb = k;
        for (int k = peak + 1; k < n && db_cmp(p, y, k, peak, &und) <= 0; ++k)
            if (db_cmp(p, y, k, rb, &und) < 0) rb = k;
        const int base = db_cmp(p, y, lb, rb, &und) >= 0 ? lb : rb;
        const double prom = y[peak] - y[base];
        if (!(fabs(prom - 6.0) > PEAK_BAND_DB)) und = 1;
        if (prom >= 6.0) {
            const int k = atomicAdd(n_list, 1);
            if (k < PEAK_LIST) list[k] = peak;
        }
    }
    und = __syncthreads_or(und);
    if (threadIdx.x == 0) {
        int m = *n_list, out = -1;
        if (!und && m <= PEAK_LIST) {
            // strongest first (insertion sort on p; equal p is a tie the host's argsort may order either way)
            for (int a = 1; a < m; ++a) {
                const int v = list[a];
                int b = a - 1;
                while (b >= 0 && p[list[b]] < p[v]) {
                    list[b + 1] = list[b];
                    --b;
                }
                list[b + 1] = v;
            }
            const double cut = m ? y[list[0]] - 20.0 : 0.0;
            int kept = 0;
            for (int a = 0; a < m; ++a) {
                const double d = y[list[a]] - cut;
                if (!(fabs(d) > PEAK_BAND_DB)) und = 1;
                if (d >= 0.0) kept = a + 1;                          // sorted: the kept ones are a prefix
            }
            for (int a = 0; a + 1 < kept && a < max_peaks; ++a)
                if (p[list[a]] == p[list[a + 1]] || !(fabs(y[list[a]] - y[list[a + 1]]) > PEAK_BAND_DB)) und = 1;
            if (!und) {
                out = kept < max_peaks ? kept : max_peaks;
                for (int a = 0; a < out; ++a) top[a] = list[a];
            }
        }
        *n_list = out;
    }
    __syncthreads();
    return *n_list;
}

// np.linspace(lo, hi, n)[k]: k * ((hi - lo) / (n - 1)) + lo, the last bin exactly hi.  The product is rounded on its own:
// under -ffp-contract=fast hipcc fuses it with the add into one FMA (1 ulp away from NumPy's two roundings), whatever the
// HIP _rn intrinsics or a `#pragma clang fp contract(off)` say; the opaque asm is what keeps the two instructions apart.
__device__ __forceinline__ double linspace_bin(double lo, double hi, int k, int n) {
    if (k == n - 1) return hi;
    const double step = (hi - lo) / (double)(n - 1);
    double prod = (double)k * step;
    asm volatile("" : "+v"(prod));
    return prod + lo;
}

// prof[f][S] float64 -> cand[f][3] = bins[peak] (strongest first, at most max_peaks <= 3), counts[f] (-1: the host decides)
__global__ __launch_bounds__(256) void k_ground_peaks(const double *prof, const double *bins, double *cand, int32_t *counts,
                                                      int S, int max_peaks, int flag_all) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *p = reinterpret_cast<double *>(smem), *y = p + S;
    __shared__ int list[PEAK_LIST];
    __shared__ int n_list, top[GROUND_COARSE];
    const long f = blockIdx.x;
    for (int i = threadIdx.x; i < S; i += 256) {
        const double v = prof[f * S + i];
        p[i] = v;
        y[i] = 20.0 * log10(v);
    }
    __syncthreads();
    const int n = pick_peaks(p, y, S, max_peaks, list, &n_list, top);
    if (threadIdx.x < GROUND_COARSE && (int)threadIdx.x < n) cand[f * GROUND_COARSE + threadIdx.x] = bins[top[threadIdx.x]];
    if (threadIdx.x == 0) counts[f] = flag_all ? -1 : n;
}

struct ZoomArgs {
    const float2 *cubes;
    const double *hann;                  // float64 Hann(S), np.hanning
    const double *cand;                  // [F][3] coarse candidates
    const int32_t *counts;               // [F]
    double *spec;                        // [F][3][S] mean |DFT| (read back by the host for flagged windows)
    double *zcand;                       // [F][3][2]
    int32_t *zcounts;                    // [F][3]
    int V, S, C, vb;
    double half, hi_cap, fs, range_max;  // zoom half width, max(range_bins) - 1e-6, 1 / range_res, range_max
    int flag_all;
};

// Altimeter._look_zoom + RangeProcessor.zoom_fft (processors/range_resp.py:59-102) around coarse candidate blockIdx.x of
// frame blockIdx.y.  The window and the bins (np.linspace) are the host's float64 expressions, rounded op by op (no
// FMA in linspace_bin: the bins are what the tracker reports).  Thread t owns bins t, t + 256, ...; each bin is the direct float64
// sum over the S windowed samples of every antenna, the phase reduced to [-1/2, 1/2] turns before sincospi.
__global__ __launch_bounds__(256) void k_ground_zoom(ZoomArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2 *xs = reinterpret_cast<double2 *>(smem);                 // [vb][S] windowed samples
    __shared__ int list[PEAK_LIST];
    __shared__ int n_list, top[GROUND_FINE];
    const int j = blockIdx.x;
    const long f = blockIdx.y, w = f * GROUND_COARSE + j;
    const int S = a.S, V = a.V;
    if (j >= a.counts[f]) {
        if (threadIdx.x == 0) a.zcounts[w] = 0;
        return;
    }
    const double c = a.cand[w];
    const double lo = fmax(1e-6, c - a.half), hi = fmin(a.hi_cap, c + a.half);       // Altimeter._look_zoom's window
    const double fstart = lo * a.fs / a.range_max, fstop = hi * a.fs / a.range_max;  // RangeProcessor.zoom_fft
    const double f0 = fstart / a.fs, df = (fstop - fstart) / (double)S / a.fs;
    double acc[ZOOM_BINS_PER_THREAD];
#pragma unroll
    for (int t = 0; t < ZOOM_BINS_PER_THREAD; ++t) acc[t] = 0.0;
    for (int v0 = 0; v0 < V; v0 += a.vb) {
        const int nv = V - v0 < a.vb ? V - v0 : a.vb;
        __syncthreads();
        for (int e = threadIdx.x; e < nv * S; e += 256) {
            const int v = e / S, i = e - v * S;
            const float2 x = a.cubes[((f * V + v0 + v) * S + i) * (long)a.C];     // chirp 0
            const double wi = a.hann[i];
            xs[e] = make_double2(__dmul_rn((double)x.x, wi), __dmul_rn((double)x.y, wi));
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < ZOOM_BINS_PER_THREAD; ++t) {
            const int k = threadIdx.x + 256 * t;
            if (k >= S) break;
            const double fk = f0 + (double)k * df;
            double re[ZOOM_VB], im[ZOOM_VB];
#pragma unroll
            for (int v = 0; v < ZOOM_VB; ++v) re[v] = im[v] = 0.0;
            for (int i = 0; i < S; ++i) {
                double turns = fk * (double)i;
                turns -= rint(turns);
                double sn, cs;
                sincospi(-2.0 * turns, &sn, &cs);
#pragma unroll
                for (int v = 0; v < ZOOM_VB; ++v) {
                    if (v < nv) {
                        const double2 x = xs[v * S + i];
                        re[v] += x.x * cs - x.y * sn;
                        im[v] += x.x * sn + x.y * cs;
                    }
                }
            }
#pragma unroll
            for (int v = 0; v < ZOOM_VB; ++v)
                if (v < nv) acc[t] += hypot(re[v], im[v]);                 // np.mean(axis=0): antennas added in order
        }
    }
    __syncthreads();                                                   // the staging area becomes p / y
    double *p = reinterpret_cast<double *>(smem), *y = p + S;
#pragma unroll
    for (int t = 0; t < ZOOM_BINS_PER_THREAD; ++t) {
        const int k = threadIdx.x + 256 * t;
        if (k >= S) break;
        const double m = acc[t] / (double)V;
        p[k] = m;
        y[k] = 20.0 * log10(m);
        a.spec[w * S + k] = m;
    }
    __syncthreads();
    const int n = pick_peaks(p, y, S, GROUND_FINE, list, &n_list, top);
    if ((int)threadIdx.x < n) a.zcand[w * GROUND_FINE + threadIdx.x] = linspace_bin(lo, hi, top[threadIdx.x], S);
    if (threadIdx.x == 0) a.zcounts[w] = a.flag_all ? -1 : n;
}

// mask[f][r][d] = the 1-D CFAR decision of Doppler bin d in range row r when row r of frame f is selected, else 0.
// Selected rows: gate[f] = (near, far), both included (rows == nullptr: the ground detector), or the ascending list
// rows[f][0 .. nrows[f]) of R-entry lists (the sequential detector's full-plane route, mmw_seq.h).
__global__ __launch_bounds__(256) void k_cfar1d_gated(Cfar1dArgs p, const int32_t *gate, const int32_t *rows, const int32_t *nrows,
                                                      uint8_t *mask, int R) {
    const long cell = (long)blockIdx.x * 256 + threadIdx.x;
    const long f = blockIdx.y;
    if (cell >= (long)R * p.L) return;
    const int r = (int)(cell / p.L), d = (int)(cell - (long)r * p.L);
    bool selected;
    if (rows == nullptr) {
        selected = r >= gate[2 * f] && r <= gate[2 * f + 1];
    } else {
        const int32_t *list = rows + f * R;
        int lo = 0, hi = nrows[f] < R ? nrows[f] : R;                // first entry >= r
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (list[mid] < r) lo = mid + 1;
            else hi = mid;
        }
        selected = lo < (nrows[f] < R ? nrows[f] : R) && list[lo] == r;
    }
    uint8_t hit = 0;
    if (selected) {
        const double *x = p.x + (f * R + r) * (long)p.L;
        double est;
        hit = x[d] > cfar1d_threshold(p, x, d, &est) ? 1 : 0;
    }
    mask[f * R * (long)p.L + cell] = hit;
}

}  // namespace mmw
