// Translation unit of the synthetic-array self-calibration (mmw_synth_calib.h): the spectra, decision and solve kernels, the entry
// that enqueues contraction - calibration - contraction without a host synchronisation, and the host-only twin of the decisions.
#include <algorithm>
#include <vector>

#include "mmw_ctx.h"
#include "mmw_fft_generic.h"
#include "mmw_synth_array.h"
#include "mmw_synth_calib.h"

namespace mmw {
// mmw_tu_synth_array.hip: the contraction kernels are instantiated there
int synth_array_contract(mmw_ctx *ctx, const char *family, const void *d_cubes, int V, int S, int C, int v, int k, int H, const int *d_frames,
                         int n_out, const double *d_P, const double *d_dirs, int T, double lambda_m, void *d_out, size_t head);
}  // namespace mmw

using namespace mmw;

namespace {

constexpr int SAC_RT = 8;               // rows of the spectrum per wave of k_sac_spectra
constexpr int SAC_RB = 4 * SAC_RT;      // ... per workgroup

__global__ __launch_bounds__(256) void k_sac_twiddles(double2 *tw, int S) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= S) return;
    double sn, cs;
    sincospi(2.0 * (double)m / (double)S, &sn, &cs);
    tw[m] = make_double2(cs, -sn);
}

// L[f][r] = sum_j 20 log10 |F_f[r][j]|, B[f][r] = sum_j l1_f[j] / |F_f[r][j]|, l1f[f] = sum_j l1_f[j] for the resident frames
// f_lo + blockIdx.x / nrb, with F_f[r][j] = sum_s x_f[s][j k] W^(r s) in float64 and l1_f[j] = sum_s |re| + |im|.  A wave owns
// SAC_RT rows and walks the columns with its lanes (coalesced for k = 1); the twiddle table sits in the LDS (16 S bytes) and the
// index of a row is the same for all lanes, so a read is one broadcast.  The products are explicit fma()s: the unit is built with
// -ffp-contract=off for the decision code, and the (S + 4) 2^-52 l1 bound of a direct sum holds with fused products as well.
__global__ __launch_bounds__(256) void k_sac_spectra(const float2 *__restrict__ X, long fs, int v, int S, int C, int k, int Cv, int f_lo,
                                                     int nrb, const double2 *__restrict__ tw, double *__restrict__ L,
                                                     double *__restrict__ B, double *__restrict__ l1f) {
    extern __shared__ __attribute__((aligned(16))) char sac_tw_smem[];
    double2 *tws = reinterpret_cast<double2 *>(sac_tw_smem);
    for (int m = threadIdx.x; m < S; m += 256) tws[m] = tw[m];
    __syncthreads();
    const int fb = blockIdx.x / nrb, rb = blockIdx.x - fb * nrb;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r0 = rb * SAC_RB + wave * SAC_RT;
    if (r0 >= S) return;        // (after the only barrier)
    const float2 *x0 = X + (long)(f_lo + fb) * fs + (long)v * S * C;
    int rq[SAC_RT];
    double ls[SAC_RT], bs[SAC_RT], l1s = 0.0;
#pragma unroll
    for (int q = 0; q < SAC_RT; ++q) {
        rq[q] = r0 + q < S ? r0 + q : S - 1;
        ls[q] = bs[q] = 0.0;
    }
    const double eps = sac_sum_eps(S);
    for (int j = lane; j < Cv; j += 64) {
        double ar[SAC_RT], ai[SAC_RT], l1 = 0.0;
        int m[SAC_RT];
#pragma unroll
        for (int q = 0; q < SAC_RT; ++q) ar[q] = ai[q] = 0.0, m[q] = 0;
        const float2 *col = x0 + (long)j * k;
        for (int s = 0; s < S; ++s) {
            const float2 xv = col[(long)s * C];
            const double xr = xv.x, xi = xv.y;
            l1 += fabs(xr) + fabs(xi);
#pragma unroll
            for (int q = 0; q < SAC_RT; ++q) {
                const double2 w = tws[m[q]];
                ar[q] = fma(xr, w.x, fma(-xi, w.y, ar[q]));
                ai[q] = fma(xr, w.y, fma(xi, w.x, ai[q]));
                m[q] += rq[q];
                if (m[q] >= S) m[q] -= S;
            }
        }
#pragma unroll
        for (int q = 0; q < SAC_RT; ++q) {
            // The error of 20 log10 |F| is bounded to first order by (20 / ln 10) eps l1 / |F|, which is sound only while the
            // relative error is small: a sum that (nearly) cancels -- integer samples at r = 0 or S / 2 cancel exactly, and are
            // then rounding noise of the tapered sum on the host -- has no bounded logarithm.  Its row gets an infinite error
            // and the frame goes to the host.  (An all-zero column is log10(0) on the host too: kept.)
            const double mag = hypot(ar[q], ai[q]);
            const bool sound = l1 == 0.0 || eps * l1 <= 0.1 * mag;
            ls[q] += sound ? 20.0 * log10(mag) : 0.0;
            bs[q] += sound ? l1 / mag : HUGE_VAL;
        }
        l1s += l1;
    }
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < SAC_RT; ++q) {
            ls[q] += __shfl_xor(ls[q], off);
            bs[q] += __shfl_xor(bs[q], off);
        }
        l1s += __shfl_xor(l1s, off);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < SAC_RT; ++q)
            if (r0 + q < S) {
                L[(long)fb * S + r0 + q] = ls[q];
                B[(long)fb * S + r0 + q] = bs[q];
            }
        if (rb == 0 && wave == 0) l1f[fb] = l1s;
    }
}

struct SacArgs {
    const float2 *X;            // the resident cubes
    long fs;
    int v, S, C, k, H, Cv, E;
    const int *frames;          // [n_out]
    int f_lo;                   // resident frame of L / B / l1f row 0
    const double *L, *B, *l1f;
    const double2 *tw;
    double hamsum;              // sum_e 20 log10 hamming(E)[e]
    const double *P, *dirs;     // the uncalibrated geometry [n_out][3][E], directions [3][T]
    int n_az, n_el, T;
    double lambda_m;
    const float2 *img;          // [n_out][S][T]: the latest image
    double *Pcal;               // [n_out][3][E]
    int *status, *targets, *state;
    double *ang, *perr;         // [n_out][3][E] each
};

__global__ __launch_bounds__(256) void k_sac_init(int *status, int *targets, int *state, int n_out, int flag_all) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    status[i] = flag_all ? -1 : 0;
    state[i] = flag_all ? SAC_FLAGGED : SAC_RUNNING;
    for (int q = 0; q < 6; ++q) targets[(long)i * 6 + q] = -1;
}

// One calibration iteration of one frame per workgroup: range rows, azimuth bins, three phase histories, the solve and the prefix
// sum.  Dynamic LDS: avg[S], err[S].  Frames that are not SAC_RUNNING are left alone.
__global__ __launch_bounds__(256) void k_sac_frame(SacArgs a) {
    extern __shared__ __attribute__((aligned(16))) char sac_smem[];
    double *avg = reinterpret_cast<double *>(sac_smem), *err = avg + a.S;
    __shared__ int sh_i[8];
    __shared__ double sh_pinv[6], sh_sum[256][2], sh_cond;
    const int i = blockIdx.x, tid = threadIdx.x;
    if (a.state[i] != SAC_RUNNING) return;
    const int S = a.S, E = a.E, w0 = a.frames[i] - a.H + 1;
    const double c_db = 20.0 / 2.302585092994046 * sac_sum_eps(S);
    for (int r = tid; r < S; r += 256) {
        double sl = 0.0, sb = 0.0;
        bool dead = false;
        for (int h = 0; h < a.H; ++h) {
            const int fr = w0 + h;
            if (fr < 0) {
                dead = true;
                continue;
            }
            sl += a.L[(long)(fr - a.f_lo) * S + r];
            sb += a.B[(long)(fr - a.f_lo) * S + r];
        }
        const double m = dead ? -HUGE_VAL : (a.hamsum + sl) / E;
        avg[r] = m;
        // the direct sums (through B), then the logarithms and the float64 mean over E values of at most 400 dB
        err[r] = dead ? 0.0 : c_db * sb / E + 1e-12 * (fabs(m) + 1.0);
    }
    __syncthreads();
    if (tid == 0) {
        int rows[3];
        sh_i[0] = sac_range_rows(avg, err, S, rows);
        sh_i[1] = rows[0], sh_i[2] = rows[1], sh_i[3] = rows[2];
    }
    __syncthreads();
    if (sh_i[0] <= 0) {
        if (tid == 0) {
            a.state[i] = sh_i[0] < 0 ? SAC_FLAGGED : SAC_STOPPED;
            if (sh_i[0] < 0) a.status[i] = -1;
        }
        return;
    }
    if (tid < 3) {
        double l1w = 0.0;
        for (int h = 0; h < a.H; ++h) l1w += a.l1f[w0 + h - a.f_lo];        // (every slot is resident: avg is finite)
        const double band = sac_image_eps(S, E) * l1w;
        sh_i[4 + tid] = sac_azimuth(SacImageLine{a.img + ((long)i * S + sh_i[1 + tid]) * a.T, a.n_el}, a.n_az, band);
    }
    __syncthreads();
    const int az[3] = {sh_i[4], sh_i[5], sh_i[6]}, row[3] = {sh_i[1], sh_i[2], sh_i[3]};
    if (az[0] < 0 || az[1] < 0 || az[2] < 0) {
        const bool flag = az[0] == -2 || az[1] == -2 || az[2] == -2;
        if (tid == 0) {
            a.state[i] = flag ? SAC_FLAGGED : SAC_STOPPED;
            if (flag) a.status[i] = -1;
        }
        return;
    }
    // the three steered phase histories: float64 direct sums over s, read in place
    const double *Pi = a.P + (long)i * 3 * E;
    double dv[3][3];
    for (int t = 0; t < 3; ++t)
        for (int c = 0; c < 3; ++c) dv[t][c] = a.dirs[(long)c * a.T + (long)az[t] * a.n_el];
    double *ang = a.ang + (long)i * 3 * E, *perr = a.perr + (long)i * 3 * E;
    for (int e = tid; e < E; e += 256) {
        const int h = e / a.Cv, j = e - h * a.Cv;
        const float2 *col = a.X + (long)(w0 + h) * a.fs + (long)a.v * S * a.C + (long)j * a.k;
        double ar[3] = {0, 0, 0}, ai[3] = {0, 0, 0}, l1 = 0.0;
        int m[3] = {0, 0, 0};
        for (int s = 0; s < S; ++s) {
            const float2 xv = col[(long)s * a.C];
            const double xr = xv.x, xi = xv.y;
            l1 += fabs(xr) + fabs(xi);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const double2 w = a.tw[m[t]];
                ar[t] = fma(xr, w.x, fma(-xi, w.y, ar[t]));
                ai[t] = fma(xr, w.y, fma(xi, w.x, ai[t]));
                m[t] += row[t];
                if (m[t] >= S) m[t] -= S;
            }
        }
        const double hm = sac_hamming(e, E);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const double raw = (dv[t][0] * Pi[e] + dv[t][1] * Pi[E + e] + dv[t][2] * Pi[2 * E + e]) / a.lambda_m;
            const double turns = raw - rint(raw);
            double sn, cs;
            sincospi(2.0 * turns, &sn, &cs);
            const double zr = hm * (ar[t] * cs - ai[t] * sn), zi = hm * (ar[t] * sn + ai[t] * cs);
            const double mag = hypot(ar[t], ai[t]);
            ang[(long)t * E + e] = atan2(zi, zr);
            // the direct sum, the steering phase as the host forms it (2 pi raw, rounded), atan2
            perr[(long)t * E + e] = (mag > 0.0 ? sac_sum_eps(S) * l1 / mag : HUGE_VAL) + 16.0 * DBL_EPSILON * (fabs(raw) + 1.0) * 2.0 * SAC_PI;
        }
    }
    if (tid == 0) {
        double D[3][2], pinv[2][3];
        for (int t = 0; t < 3; ++t)
            for (int c = 0; c < 2; ++c) D[t][c] = 2.0 * SAC_PI / a.lambda_m * dv[t][c];
        sh_cond = sac_pinv(D, pinv);
        for (int q = 0; q < 6; ++q) sh_pinv[q] = pinv[q / 3][q % 3];
    }
    __threadfence_block();
    __syncthreads();
    if (!(sh_cond <= SAC_COND_MAX)) {
        if (tid == 0) a.state[i] = SAC_FLAGGED, a.status[i] = -1;
        return;
    }
    // delta of the steps [e0, e1) of this thread, twice: once for the chunk sums, once with the offset for the stores
    const int n = E - 1, ch = (n + 255) / 256;
    const int e0 = tid * ch < n ? tid * ch : n, e1 = e0 + ch < n ? e0 + ch : n;
    bool near = false;
    double sx = 0.0, sy = 0.0;
    for (int e = e0; e < e1; ++e) {
        double ph[3];
        for (int t = 0; t < 3; ++t)
            ph[t] = sac_phase_step(ang[(long)t * E + e], ang[(long)t * E + e + 1], perr[(long)t * E + e] + perr[(long)t * E + e + 1], &near);
        sx += sh_pinv[0] * ph[0] + sh_pinv[1] * ph[1] + sh_pinv[2] * ph[2];
        sy += sh_pinv[3] * ph[0] + sh_pinv[4] * ph[1] + sh_pinv[5] * ph[2];
    }
    sh_sum[tid][0] = sx, sh_sum[tid][1] = sy;
    if (__syncthreads_or(near)) {
        if (tid == 0) a.state[i] = SAC_FLAGGED, a.status[i] = -1;
        return;
    }
    if (tid == 0) {             // exclusive scan of the chunk sums, in order
        double cx = 0.0, cy = 0.0;
        for (int q = 0; q < 256; ++q) {
            const double x = sh_sum[q][0], y = sh_sum[q][1];
            sh_sum[q][0] = cx, sh_sum[q][1] = cy;
            cx += x, cy += y;
        }
    }
    __syncthreads();
    double cx = sh_sum[tid][0], cy = sh_sum[tid][1];
    double *Pc = a.Pcal + (long)i * 3 * E;
    bool unused = false;
    for (int e = e0; e < e1; ++e) {
        double ph[3];
        for (int t = 0; t < 3; ++t) ph[t] = sac_phase_step(ang[(long)t * E + e], ang[(long)t * E + e + 1], 0.0, &unused);
        cx += sh_pinv[0] * ph[0] + sh_pinv[1] * ph[1] + sh_pinv[2] * ph[2];
        cy += sh_pinv[3] * ph[0] + sh_pinv[4] * ph[1] + sh_pinv[5] * ph[2];
        Pc[e + 1] = Pi[e + 1] - cx;
        Pc[E + e + 1] = Pi[E + e + 1] - cy;
    }
    if (tid == 0) {
        a.status[i] += 1;
        for (int t = 0; t < 3; ++t) a.targets[(long)i * 6 + 2 * t] = row[t], a.targets[(long)i * 6 + 2 * t + 1] = az[t];
    }
}

// array_geometry_calibrated of a frame whose loop stopped, or that goes to the host, is the uncalibrated geometry; a flagged frame
// (whatever iteration flagged it) reports no targets: the host decides them
__global__ __launch_bounds__(256) void k_sac_finish(const int *state, const double *P, double *Pcal, int *targets, int E) {
    const long i = blockIdx.x;
    if (state[i] == SAC_RUNNING) return;
    for (int q = threadIdx.x; q < 3 * E; q += 256) Pcal[i * 3 * E + q] = P[i * 3 * E + q];
    if (state[i] == SAC_FLAGGED && threadIdx.x < 6) targets[i * 6 + threadIdx.x] = -1;
}

// static (sh_i, sh_pinv, sh_sum, sh_cond) + dynamic LDS of k_sac_frame, and the table of k_sac_spectra, stay inside the 64 KiB a
// launch gets without asking for more
static_assert(16 * SAC_MAX_S + 8 * 4 + 8 * (6 + 512 + 1) + 256 <= 64 * 1024, "k_sac_frame: avg, err and the static arrays exceed 64 KiB");

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

int sac_validate(int n_iters, const void *d_Pcal, const void *d_status, const void *d_targets) {
    MMW_REQUIRE(d_Pcal && d_status && d_targets, "null argument (d_Pcal %d, d_status %d, d_targets %d)", d_Pcal != nullptr,
                d_status != nullptr, d_targets != nullptr);
    MMW_REQUIRE(n_iters >= 1 && n_iters <= 8, "n_iters %d is not in [1, 8]", n_iters);
    return MMW_OK;
}

}  // namespace

extern "C" {

int mmw_synth_array_calibrate(mmw_ctx *ctx, const void *d_cubes, int n_resident, int V, int S, int C, int v, int k, int H,
                              const int32_t *h_frames, int n_out, const double *h_P, const double *h_dirs, int n_az, int n_el,
                              double lambda_m, int n_iters, void *d_out, double *d_Pcal, int32_t *d_status, int32_t *d_targets) {
    MMW_REQUIRE(n_az >= 1 && n_el >= 1 && (long)n_az * n_el <= INT32_MAX, "%d azimuth x %d elevation bins are not a direction count", n_az, n_el);
    const int T = n_az * n_el;
    MMW_TRY(sa_validate(ctx != nullptr, d_cubes, n_resident, V, S, C, v, k, H, h_frames, n_out, h_P, h_dirs, T, lambda_m, d_out));
    MMW_TRY(sac_validate(n_iters, d_Pcal, d_status, d_targets));
    if (S > SAC_MAX_S) return set_error(MMW_ERR_UNSUPPORTED, "the calibration keeps avg[S] in the LDS: S %d is more than %d", S, SAC_MAX_S);
    if (n_out == 0) return MMW_OK;
    const int Cv = sa_cv(C, k), E = H * Cv;
    const int f_lo = std::max(0, h_frames[0] - H + 1), nf = h_frames[n_out - 1] - f_lo + 1, nrb = (S + SAC_RB - 1) / SAC_RB;
    if ((long)nf * nrb > INT32_MAX) return set_error(MMW_ERR_UNSUPPORTED, "%d frames x %d row blocks do not fit one grid", nf, nrb);
    MMW_JOIN(ctx);
    ProfScope ps(ctx, "synth_calib");
    // the head of the scratch: mmw_synth_array's tables, then this call's
    size_t off = sa_head_bytes(n_out, E, T);
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += up256(bytes);
        return at;
    };
    const size_t o_L = take((size_t)nf * S * 8), o_B = take((size_t)nf * S * 8), o_l1 = take((size_t)nf * 8), o_tw = take((size_t)S * 16);
    const size_t o_state = take((size_t)n_out * 4), o_ang = take((size_t)n_out * 3 * E * 8), o_perr = take((size_t)n_out * 3 * E * 8);
    const size_t head = off;
    SaStaged st;
    MMW_TRY(sa_stage(ctx, S, E, T, h_frames, n_out, h_P, h_dirs, head, &st));
    char *base = (char *)ctx->scratch;
    double hamsum = 0.0;
    for (int e = 0; e < E; ++e) hamsum += 20.0 * std::log10(sac_hamming(e, E));
    SacArgs a{};
    a.X = (const float2 *)d_cubes, a.fs = (long)V * S * C;
    a.v = v, a.S = S, a.C = C, a.k = k, a.H = H, a.Cv = Cv, a.E = E;
    a.frames = st.d_frames, a.f_lo = f_lo;
    a.L = (double *)(base + o_L), a.B = (double *)(base + o_B), a.l1f = (double *)(base + o_l1), a.tw = (double2 *)(base + o_tw);
    a.hamsum = hamsum;
    a.P = st.d_P, a.dirs = st.d_dirs, a.n_az = n_az, a.n_el = n_el, a.T = T, a.lambda_m = lambda_m;
    a.img = (const float2 *)d_out, a.Pcal = d_Pcal, a.status = d_status, a.targets = d_targets, a.state = (int *)(base + o_state);
    a.ang = (double *)(base + o_ang), a.perr = (double *)(base + o_perr);
    {
        ProfScope pq(ctx, "synth_calib_spectra");
        hipLaunchKernelGGL(k_sac_twiddles, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, (double2 *)(base + o_tw), S);
        MMW_TRY(check_launch("sac_twiddles"));
        hipLaunchKernelGGL(k_sac_spectra, dim3((unsigned)((long)nf * nrb)), dim3(256), (size_t)S * 16, ctx->stream, a.X, a.fs, v, S, C, k, Cv, f_lo, nrb,
                           a.tw, (double *)(base + o_L), (double *)(base + o_B), (double *)(base + o_l1));
        MMW_TRY(check_launch("sac_spectra"));
    }
    hipLaunchKernelGGL(k_sac_init, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, ctx->stream, d_status, d_targets, a.state, n_out,
                       opt_int(ctx, "MMW_SYNTH_CALIB_FLAG_ALL", 0) != 0);
    MMW_TRY(check_launch("sac_init"));
    MMW_HIP(hipMemcpyAsync(d_Pcal, st.d_P, (size_t)n_out * 3 * E * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    MMW_TRY(synth_array_contract(ctx, "synth_array", d_cubes, V, S, C, v, k, H, st.d_frames, n_out, st.d_P, st.d_dirs, T, lambda_m, d_out, head));
    for (int it = 0; it < n_iters; ++it) {
        {
            ProfScope pq(ctx, "synth_calib_frame");
            hipLaunchKernelGGL(k_sac_frame, dim3((unsigned)n_out), dim3(256), (size_t)S * 16, ctx->stream, a);
            MMW_TRY(check_launch("sac_frame"));
        }
        MMW_TRY(synth_array_contract(ctx, "synth_array", d_cubes, V, S, C, v, k, H, st.d_frames, n_out, d_Pcal, st.d_dirs, T, lambda_m, d_out, head));
    }
    hipLaunchKernelGGL(k_sac_finish, dim3((unsigned)n_out), dim3(256), 0, ctx->stream, a.state, st.d_P, d_Pcal, d_targets, E);
    return check_launch("sac_finish");
}

// Steps 3-6 on host pointers, one window, one iteration: h_avg [S] (+- h_avg_err [S], or null: exact), h_mag [S][n_az] the image
// magnitudes at elevation 0 (+- mag_band), h_Fq [S][E] complex128 of which the three picked rows are read, h_l1 [E] the L1 norms
// of the columns behind the phase error bound (or null: exact), h_P [3][E], h_dirs [3][n_az n_el].  h_Pcal [3][E] gets the
// corrected geometry (the uncalibrated one unless info[0] is 1), h_targets [3][2] the picks (-1: none), info = {1 applied /
// 0 no suitable targets / -1 flagged, SAC_WHY_* bits, range peaks found (3 or 0), condition number > 1e6}.
int mmw_diag_synth_array_calib_host(const double *h_avg, const double *h_avg_err, int S, const double *h_mag, double mag_band, int n_az,
                                    int n_el, const double *h_Fq, const double *h_l1, int E, const double *h_P, const double *h_dirs,
                                    double lambda_m, double *h_Pcal, int32_t *h_targets, int32_t info[4]) {
    MMW_REQUIRE(h_avg && h_mag && h_Fq && h_P && h_dirs && h_Pcal && h_targets && info, "null argument");
    MMW_REQUIRE(S >= 1 && E >= 1 && n_az >= 1 && n_el >= 1 && (long)n_az * n_el <= INT32_MAX, "bad shape: S %d, E %d, n_az %d, n_el %d", S, E,
                n_az, n_el);
    MMW_REQUIRE(lambda_m > 0.0, "lambda_m %g is not positive", lambda_m);
    MMW_REQUIRE(mag_band >= 0.0, "mag_band %g is negative", mag_band);
    const long T = (long)n_az * n_el;
    for (long q = 0; q < 3L * E; ++q) h_Pcal[q] = h_P[q];
    for (int q = 0; q < 6; ++q) h_targets[q] = -1;
    info[0] = info[1] = info[2] = info[3] = 0;
    std::vector<double> zero_err;
    if (!h_avg_err) {
        zero_err.assign((size_t)S, 0.0);
        h_avg_err = zero_err.data();
    }
    int rows[3];
    const int rc = sac_range_rows(h_avg, h_avg_err, S, rows);
    if (rc < 0) {
        info[0] = -1, info[1] = SAC_WHY_RANGE;
        return MMW_OK;
    }
    if (rc == 0) return MMW_OK;
    info[2] = 3;
    int az[3], n_t = 0;
    for (int t = 0; t < 3; ++t) {
        az[t] = sac_azimuth(SacLine{h_mag + (long)rows[t] * n_az, 1}, n_az, mag_band);
        if (az[t] == -2) {
            info[0] = -1, info[1] = SAC_WHY_AZIMUTH;
            return MMW_OK;
        }
        n_t += az[t] >= 0;
    }
    if (n_t < 3) return MMW_OK;
    double D[3][2], pinv[2][3];
    for (int t = 0; t < 3; ++t)
        for (int c = 0; c < 2; ++c) D[t][c] = 2.0 * SAC_PI / lambda_m * h_dirs[c * T + (long)az[t] * n_el];
    const double cond = sac_pinv(D, pinv);
    info[3] = !(cond <= SAC_COND_MAX);
    std::vector<double> ang((size_t)3 * E), perr((size_t)3 * E, 0.0);
    for (int t = 0; t < 3; ++t)
        for (int e = 0; e < E; ++e) {
            const double fr = h_Fq[2 * ((long)rows[t] * E + e)], fi = h_Fq[2 * ((long)rows[t] * E + e) + 1];
            double raw = 0.0;
            for (int c = 0; c < 3; ++c) raw += h_dirs[c * T + (long)az[t] * n_el] * h_P[(long)c * E + e];
            raw /= lambda_m;
            const double th = 2.0 * SAC_PI * (raw - std::rint(raw)), cs = std::cos(th), sn = std::sin(th);
            ang[(size_t)t * E + e] = std::atan2(fr * sn + fi * cs, fr * cs - fi * sn);
            if (h_l1) {
                const double mag = std::hypot(fr, fi);
                perr[(size_t)t * E + e] = (mag > 0.0 ? sac_sum_eps(S) * sac_hamming(e, E) * h_l1[e] / mag : HUGE_VAL) +
                                          16.0 * DBL_EPSILON * (std::fabs(raw) + 1.0) * 2.0 * SAC_PI;
            }
        }
    bool near = false;
    std::vector<double> corr((size_t)2 * std::max(E - 1, 1));
    double cx = 0.0, cy = 0.0;
    for (int e = 0; e + 1 < E; ++e) {
        double ph[3];
        for (int t = 0; t < 3; ++t)
            ph[t] = sac_phase_step(ang[(size_t)t * E + e], ang[(size_t)t * E + e + 1], perr[(size_t)t * E + e] + perr[(size_t)t * E + e + 1], &near);
        cx += pinv[0][0] * ph[0] + pinv[0][1] * ph[1] + pinv[0][2] * ph[2];
        cy += pinv[1][0] * ph[0] + pinv[1][1] * ph[1] + pinv[1][2] * ph[2];
        corr[(size_t)e] = cx, corr[(size_t)(E - 1) + e] = cy;
    }
    if (near || info[3]) info[0] = -1, info[1] = (near ? SAC_WHY_WRAP : 0) | (info[3] ? SAC_WHY_COND : 0);
    if (near) return MMW_OK;
    // (an ill-conditioned D is flagged AND solved: the minimum-norm solution is what the host route returns for it)
    for (int e = 0; e + 1 < E; ++e) {
        h_Pcal[e + 1] = h_P[e + 1] - corr[(size_t)e];
        h_Pcal[(long)E + e + 1] = h_P[(long)E + e + 1] - corr[(size_t)(E - 1) + e];
    }
    for (int t = 0; t < 3; ++t) h_targets[2 * t] = rows[t], h_targets[2 * t + 1] = az[t];
    if (info[0] == 0) info[0] = 1;
    return MMW_OK;
}

}  // extern "C"
