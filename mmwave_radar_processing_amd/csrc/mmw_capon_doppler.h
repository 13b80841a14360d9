// MVDR-beamformed Doppler of Capon detections (mmw_capon_doppler): for a detection (q, t) on the Capon
// range-azimuth map of a frame, with X [n][R][K] the frame's snapshots widened exactly to float64,
//   R_q = X_q X_q^H / K + delta tr(X_q X_q^H / K) / n I,   u = R_q^-1 a(theta_t),   w = u / Re(a^H u),
//   y[k] = sum_i conj(w_i) X[i][q][k],   z = fftshift(DFT_K(h y)),   dop = first index of max |z|,   peak = |z[dop]|.
//
//   cd_*            the arithmetic, ONE __host__ __device__ implementation: k_capon_doppler and the host-only entry
//                   mmw_diag_capon_doppler_host call the same functions, and every sum runs in the same order in both (this unit is
//                   built with -ffp-contract=off), so the two agree bit for bit.
//   k_cd_fill       one lane per detection slot: slots past the frame's count are zeroed, a detection whose q or t is out of range
//                   gets dop -1 / NaN.  Every other slot is left to k_capon_doppler.
//   k_capon_doppler one workgroup per (frame, range row).  It reads the frame's detection list 256 entries at a time and keeps the
//                   entries of its row; a row without detections ends there.  On the first hit the workgroup loads the row's
//                   snapshots, the twiddles and the window into the LDS, accumulates R_q (one lane per entry, K terms), factors it
//                   (Cholesky, one lane per row of the column, n steps) and inverts it (one lane per column: two triangular
//                   solves).  The row's detections then go in chunks of `ch`: u = R_q^-1 a (one lane per (detection, antenna)),
//                   the weights, y (one lane per (detection, chirp)), the K-point direct DFT with the twiddle index (k d) mod K
//                   stepped in integers (one lane per (detection, Doppler bin)), and the argmax by 16 lanes per detection.
//
// No libm call runs on the device: steering vectors, cos / sin of the angles, twiddles and the window are float64 tables made on
// the host.  sqrt and the divisions are the correctly rounded IEEE operations.  Vector stores only.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/mmwgpu.h"

namespace mmw {

constexpr int CD_MAX_N = 16;            // antennas
constexpr int CD_MAX_K = 512;           // chirps
constexpr int CD_THREADS = 256;
constexpr int CD_MP = CD_MAX_N + 1;     // pitch of the n x n matrices, in complex128 entries
constexpr int CD_MAX_CHUNK = 16;        // detections of a row carried at once (16 lanes each in the argmax: CD_THREADS / 16)
constexpr int CD_CHUNK_CELLS = 512;     // ... and at most this many (detection, chirp) cells: 12 KiB of y and |z|

struct CdC {
    double re, im;
};

inline int cd_chunk(int K) {
    const int ch = CD_CHUNK_CELLS / K;
    return ch < 1 ? 1 : (ch > CD_MAX_CHUNK ? CD_MAX_CHUNK : ch);
}

// Row q of the snapshots: element (i, k) of X[n][R][K] in host or device memory, or of the [n][K + 1] LDS copy
struct CdSnap {
    const float2 *p;
    long ant_stride;
    __host__ __device__ CdC operator()(int i, int k) const {
        const float2 v = p[i * ant_stride + k];
        return CdC{(double)v.x, (double)v.y};
    }
};

// Entry (i, j), i >= j, of X_q X_q^H / K: K terms in chirp order
__host__ __device__ inline CdC cd_cov_entry(const CdSnap &X, int i, int j, int K) {
    double sr = 0.0, si = 0.0;
    for (int k = 0; k < K; ++k) {
        const CdC a = X(i, k), b = X(j, k);
        sr += a.re * b.re + a.im * b.im;
        si += a.im * b.re - a.re * b.im;
    }
    return CdC{sr / (double)K, si / (double)K};
}

// Diagonal loading of the lower triangle A (pitch CD_MP): A_ii += delta tr(A) / n
__host__ __device__ inline void cd_load_diagonal(CdC *A, int n, double delta) {
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += A[i * CD_MP + i].re;
    const double load = delta * tr / (double)n;
    for (int i = 0; i < n; ++i) A[i * CD_MP + i].re += load;
}

// Entry (i, j), i >= j, of the Cholesky factor L (A = L L^H) from A and the columns < j of L.  Every caller of column j
// evaluates the pivot d_j itself, so a column needs no exchange inside it.  *pivot = d_j (the row is degenerate unless
// 0 < d_j < inf).
__host__ __device__ inline CdC cd_chol_entry(const CdC *A, const CdC *L, int i, int j, double *pivot) {
    double d = A[j * CD_MP + j].re;
    for (int p = 0; p < j; ++p) {
        const CdC l = L[j * CD_MP + p];
        d -= l.re * l.re + l.im * l.im;
    }
    *pivot = d;
    const double ljj = sqrt(d);
    if (i == j) return CdC{ljj, 0.0};
    CdC s = A[i * CD_MP + j];
    for (int p = 0; p < j; ++p) {
        const CdC a = L[i * CD_MP + p], b = L[j * CD_MP + p];     // s -= a conj(b)
        s.re -= a.re * b.re + a.im * b.im;
        s.im -= a.im * b.re - a.re * b.im;
    }
    return CdC{s.re / ljj, s.im / ljj};
}

__host__ __device__ inline bool cd_pivot_ok(double d) { return d > 0.0 && d <= 1.79769313486231570815e308; }

// Column c of (L L^H)^-1 into column c of M (pitch CD_MP): L v = e_c forwards, L^H x = v backwards, in place
__host__ __device__ inline void cd_inverse_column(const CdC *L, CdC *M, int n, int c) {
    for (int i = 0; i < n; ++i) {
        CdC s = CdC{i == c ? 1.0 : 0.0, 0.0};
        for (int p = 0; p < i; ++p) {
            const CdC l = L[i * CD_MP + p], v = M[p * CD_MP + c];     // s -= l v
            s.re -= l.re * v.re - l.im * v.im;
            s.im -= l.re * v.im + l.im * v.re;
        }
        const double d = L[i * CD_MP + i].re;
        M[i * CD_MP + c] = CdC{s.re / d, s.im / d};
    }
    for (int i = n - 1; i >= 0; --i) {
        CdC s = M[i * CD_MP + c];
        for (int p = i + 1; p < n; ++p) {
            const CdC l = L[p * CD_MP + i], x = M[p * CD_MP + c];     // s -= conj(l) x
            s.re -= l.re * x.re + l.im * x.im;
            s.im -= l.re * x.im - l.im * x.re;
        }
        const double d = L[i * CD_MP + i].re;
        M[i * CD_MP + c] = CdC{s.re / d, s.im / d};
    }
}

// u_i = sum_j M_ij a_j, antenna order
__host__ __device__ inline CdC cd_solve_entry(const CdC *M, const CdC *a, int n, int i) {
    CdC s = CdC{0.0, 0.0};
    for (int j = 0; j < n; ++j) {
        const CdC m = M[i * CD_MP + j], v = a[j];
        s.re += m.re * v.re - m.im * v.im;
        s.im += m.re * v.im + m.im * v.re;
    }
    return s;
}

// Re(a^H u)
__host__ __device__ inline double cd_denominator(const CdC *a, const CdC *u, int n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += a[i].re * u[i].re + a[i].im * u[i].im;
    return s;
}

// y[k] = sum_i conj(w_i) X[i][k], times the window
__host__ __device__ inline CdC cd_beamform(const CdSnap &X, const CdC *w, int n, int k, const double *hann) {
    CdC s = CdC{0.0, 0.0};
    for (int i = 0; i < n; ++i) {
        const CdC x = X(i, k), c = w[i];
        s.re += c.re * x.re + c.im * x.im;
        s.im += c.re * x.im - c.im * x.re;
    }
    if (hann) s = CdC{s.re * hann[k], s.im * hann[k]};
    return s;
}

// |z[m]| of z = fftshift(DFT_K(y)): the bin of frequency d = (m - K / 2) mod K, twiddle index (k d) mod K in integers
__host__ __device__ inline double cd_spectrum(const CdC *y, const CdC *tw, int K, int m) {
    const int d = (m + K - K / 2) % K;
    double sr = 0.0, si = 0.0;
    int idx = 0;
    for (int k = 0; k < K; ++k) {
        const CdC v = y[k], t = tw[idx];
        sr += v.re * t.re - v.im * t.im;
        si += v.re * t.im + v.im * t.re;
        idx += d;
        if (idx >= K) idx -= K;
    }
    return sqrt(sr * sr + si * si);
}

// np.argmax's order on (value, index) pairs: the larger value, the smaller index among equals.  A NaN never wins.
__host__ __device__ inline bool cd_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

__host__ __device__ inline double cd_nan() { return __builtin_nan(""); }

struct CdArgs {
    const float2 *X;            // [F][n][R][K]
    const int32_t *dets;        // [F][cap][2] (row, angle index)
    const int32_t *counts;      // [F]
    const CdC *steer;           // [T][n]
    const double *cos_t, *sin_t;    // [T]
    const CdC *tw;              // [K] exp(-2 pi j m / K)
    const double *hann;         // [K] or nullptr
    const double *range, *vel;  // [R], [K]; read only with points
    int32_t *dop;               // [F][cap]
    double *peak;               // [F][cap]
    double *spec;               // nullptr or [F][cap][K]
    double *points;             // nullptr or [F][cap][4]
    int n, R, K, T, cap, ch;
    double delta;
};

__host__ __device__ inline int cd_clamp_count(int c, int cap) { return c < 0 ? 0 : (c > cap ? cap : c); }

// What one detection's outputs are once its spectrum is known (or its row found degenerate: dop < 0)
__host__ __device__ inline void cd_point(const CdArgs &a, long slot, int q, int t, int dop, double *out4) {
    out4[0] = a.range[q] * a.cos_t[t];
    out4[1] = a.range[q] * a.sin_t[t];
    out4[2] = 0.0;
    out4[3] = dop >= 0 ? a.vel[dop] : cd_nan();
}

// grid ceil(F cap / 256): slots past the count -> zeros (the spectra are zeroed by the caller's memset), a detection outside
// [0, R) x [0, T) -> -1 / NaN
__global__ __launch_bounds__(256) void k_cd_fill(CdArgs a, long n_slots) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_slots) return;
    const long f = s / a.cap;
    const int j = (int)(s - f * a.cap);
    const bool past = j >= cd_clamp_count(a.counts[f], a.cap);
    if (!past) {
        const int q = a.dets[2 * s], t = a.dets[2 * s + 1];
        if ((unsigned)q < (unsigned)a.R && (unsigned)t < (unsigned)a.T) return;
    }
    const double v = past ? 0.0 : cd_nan();
    a.dop[s] = past ? 0 : -1;
    a.peak[s] = v;
    if (a.points) *(reinterpret_cast<double4 *>(a.points) + s) = make_double4(v, v, 0.0, v);
    if (a.spec && !past)
        for (int m = 0; m < a.K; ++m) a.spec[s * a.K + m] = v;
}

// The LDS image of k_capon_doppler, in bytes from a 16-byte aligned base
struct CdLds {
    size_t x, tw, hann, A, L, u, steer, y, mag, den, lj, lt, head, total;
};
__host__ __device__ inline CdLds cd_lds(int n, int K, int ch) {
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    CdLds o;
    size_t at = 0;
    o.head = at, at += 16;                                       // hits of the pass, degenerate flag
    o.x = at, at += up((size_t)n * (K + 1) * sizeof(float2));      // odd pitch: the rows of one chirp lie in n different banks
    o.tw = at, at += (size_t)K * sizeof(CdC);
    o.hann = at, at += up((size_t)K * sizeof(double));
    o.A = at, at += (size_t)CD_MAX_N * CD_MP * sizeof(CdC);
    o.L = at, at += (size_t)CD_MAX_N * CD_MP * sizeof(CdC);
    o.u = at, at += (size_t)ch * CD_MP * sizeof(CdC);
    o.steer = at, at += (size_t)ch * CD_MP * sizeof(CdC);
    o.y = at, at += (size_t)ch * K * sizeof(CdC);
    o.mag = at, at += (size_t)ch * K * sizeof(double);
    o.den = at, at += (size_t)CD_MAX_CHUNK * sizeof(double);
    o.lj = at, at += (size_t)CD_THREADS * sizeof(int);
    o.lt = at, at += (size_t)CD_THREADS * sizeof(int);
    o.total = at;
    return o;
}

// grid F * R, CD_THREADS threads, cd_lds(n, K, ch).total bytes of dynamic LDS
__global__ __launch_bounds__(CD_THREADS) void k_capon_doppler(CdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char cd_smem[];
    const int tid = threadIdx.x, n = a.n, K = a.K, ch = a.ch;
    const CdLds o = cd_lds(n, K, ch);
    int *head = reinterpret_cast<int *>(cd_smem + o.head);         // [0] hits of this pass, [1] the row is degenerate
    float2 *xs = reinterpret_cast<float2 *>(cd_smem + o.x);
    CdC *tw = reinterpret_cast<CdC *>(cd_smem + o.tw);
    double *hann = reinterpret_cast<double *>(cd_smem + o.hann);
    CdC *A = reinterpret_cast<CdC *>(cd_smem + o.A);
    CdC *L = reinterpret_cast<CdC *>(cd_smem + o.L);
    CdC *u = reinterpret_cast<CdC *>(cd_smem + o.u);
    CdC *st = reinterpret_cast<CdC *>(cd_smem + o.steer);
    CdC *y = reinterpret_cast<CdC *>(cd_smem + o.y);
    double *mag = reinterpret_cast<double *>(cd_smem + o.mag);
    double *den = reinterpret_cast<double *>(cd_smem + o.den);
    int *lj = reinterpret_cast<int *>(cd_smem + o.lj);
    int *lt = reinterpret_cast<int *>(cd_smem + o.lt);

    const long f = blockIdx.x / a.R;
    const int q = (int)(blockIdx.x - f * a.R);
    const int nf = cd_clamp_count(a.counts[f], a.cap);
    const int32_t *dets = a.dets + 2 * f * (long)a.cap;
    const CdSnap X{xs, K + 1};
    bool ready = false;
    for (int base = 0; base < nf; base += CD_THREADS) {
        if (tid == 0) head[0] = 0;
        __syncthreads();
        const int j = base + tid;
        if (j < nf) {
            const int dq = dets[2 * j], dt = dets[2 * j + 1];
            if (dq == q && (unsigned)dt < (unsigned)a.T) {
                const int s = atomicAdd(&head[0], 1);       // an LDS counter; the order of the hits does not reach any result
                lj[s] = j;
                lt[s] = dt;
            }
        }
        __syncthreads();
        const int hits = head[0];
        __syncthreads();                    // head[0] is zeroed again at the top of the loop
        if (hits == 0) continue;
        if (!ready) {
            ready = true;
            // the row's snapshots, the twiddles and the window
            const float2 *src = a.X + (f * n * (long)a.R + q) * (long)K;
            for (int e = tid; e < n * K; e += CD_THREADS) {
                const int i = e / K, k = e - i * K;
                xs[i * (K + 1) + k] = src[(long)i * a.R * K + k];
            }
            for (int k = tid; k < K; k += CD_THREADS) {
                tw[k] = a.tw[k];
                if (a.hann) hann[k] = a.hann[k];
            }
            if (tid == 0) head[1] = 0;
            __syncthreads();
            for (int e = tid; e < n * n; e += CD_THREADS) {
                const int i = e / n, c = e - i * n;
                if (i >= c) A[i * CD_MP + c] = cd_cov_entry(X, i, c, K);
            }
            __syncthreads();
            if (tid == 0) cd_load_diagonal(A, n, a.delta);
            __syncthreads();
            for (int c = 0; c < n; ++c) {
                if (tid >= c && tid < n) {
                    double pivot;
                    L[tid * CD_MP + c] = cd_chol_entry(A, L, tid, c, &pivot);
                    if (tid == c && !cd_pivot_ok(pivot)) head[1] = 1;
                }
                __syncthreads();
            }
            if (tid < n) cd_inverse_column(L, A, n, tid);        // A becomes R_q^-1
            __syncthreads();
        }
        const bool bad = head[1] != 0;
        for (int c0 = 0; c0 < hits; c0 += ch) {
            const int mc = hits - c0 < ch ? hits - c0 : ch;
            if (!bad) {
                for (int e = tid; e < mc * n; e += CD_THREADS) {
                    const int c = e / n, i = e - c * n;
                    st[c * CD_MP + i] = a.steer[(long)lt[c0 + c] * n + i];
                }
                __syncthreads();
                for (int e = tid; e < mc * n; e += CD_THREADS) {
                    const int c = e / n, i = e - c * n;
                    u[c * CD_MP + i] = cd_solve_entry(A, st + c * CD_MP, n, i);
                }
                __syncthreads();
                if (tid < mc) den[tid] = cd_denominator(st + tid * CD_MP, u + tid * CD_MP, n);
                __syncthreads();
                for (int e = tid; e < mc * n; e += CD_THREADS) {
                    const int c = e / n, i = e - c * n;
                    const CdC v = u[c * CD_MP + i];
                    u[c * CD_MP + i] = CdC{v.re / den[c], v.im / den[c]};
                }
                __syncthreads();
                for (int e = tid; e < mc * K; e += CD_THREADS) {
                    const int c = e / K, k = e - c * K;
                    y[c * K + k] = cd_beamform(X, u + c * CD_MP, n, k, a.hann ? hann : nullptr);
                }
                __syncthreads();
                for (int e = tid; e < mc * K; e += CD_THREADS) {
                    const int c = e / K, m = e - c * K;
                    mag[c * K + m] = cd_spectrum(y + c * K, tw, K, m);
                }
                __syncthreads();
            }
            // 16 lanes per detection: each takes the bins sub, sub + 16, ... in ascending order, then the 16 are merged
            const int c = tid >> 4, sub = tid & 15;
            double bv = -1.0;
            int bi = INT_MAX;
            if (!bad && c < mc)
                for (int m = sub; m < K; m += 16) {
                    const double v = mag[c * K + m];
                    if (cd_better(v, m, bv, bi)) bv = v, bi = m;
                }
            for (int off = 8; off >= 1; off >>= 1) {
                const double ov = __shfl_xor(bv, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (cd_better(ov, oi, bv, bi)) bv = ov, bi = oi;
            }
            if (c < mc && sub == 0) {
                const long slot = f * (long)a.cap + lj[c0 + c];
                const int dop = bi == INT_MAX ? -1 : bi;
                a.dop[slot] = dop;
                a.peak[slot] = dop < 0 ? cd_nan() : bv;
                if (a.points) {
                    double p[4];
                    cd_point(a, slot, q, lt[c0 + c], dop, p);
                    *(reinterpret_cast<double4 *>(a.points) + slot) = make_double4(p[0], p[1], p[2], p[3]);
                }
            }
            if (a.spec)
                for (int e = tid; e < mc * K; e += CD_THREADS) {
                    const int cc = e / K, m = e - cc * K;
                    a.spec[(f * (long)a.cap + lj[c0 + cc]) * K + m] = bad ? cd_nan() : mag[cc * K + m];
                }
            __syncthreads();            // y, |z| and the steering rows are rewritten by the next chunk
        }
    }
}

}  // namespace mmw
