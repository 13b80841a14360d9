/*
 * mmwgpu.h -- C ABI of libmmwgpu.so: MI355X (gfx950) range-Doppler-angle + CFAR hot path.
 *
 * Drop-in boundary for davidmhunt/mmwave_radar_processing.  The reference has no FFI
 * (SURVEY.md section 8b): its boundary is the Python class protocol
 * `processor.process(adc_cube, **kw)` / `detector.detect(x)`.  This header is what a
 * ctypes binding for that protocol binds; every entry point cites the reference
 * call (file:line, relative to mmwave_radar_processing/) whose NumPy arithmetic it replaces.
 * INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  Every function returns an int
 *     status (MMW_OK == 0, negative == error); mmw_last_error() gives the text
 *     of the calling thread's last failure.
 *   - complex64 = interleaved (re, im) float pairs.  Cube layout is the reference's:
 *     [frame][virtRx V][sample S][chirp C], C-order, chirp fastest
 *     (processors/_processor.py:58).
 *   - Pointers named d_* are DEVICE pointers obtained from mmw_malloc; h_* are host.
 *   - All compute entry points enqueue on the context's HIP stream and return
 *     without synchronising unless they take a host output pointer; call
 *     mmw_sync() before reading device results through mmw_memcpy_d2h (which
 *     synchronises itself).
 *   - One context per host thread; contexts are not thread-safe.
 */
#ifndef MMWGPU_H
#define MMWGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMW_OK                 0
#define MMW_ERR_INVALID       -1   /* bad argument (shape, null pointer, unsupported size)   */
#define MMW_ERR_HIP           -2   /* HIP runtime error, see mmw_last_error()               */
#define MMW_ERR_NOMEM         -3   /* device allocation failed                              */
#define MMW_ERR_TRUNCATED     -4   /* detection output capacity too small; counts are exact */
#define MMW_ERR_UNSUPPORTED   -5   /* valid request this build has no kernel for            */

typedef struct mmw_ctx mmw_ctx;

/* CFAR kinds: string keys of detectors/detector_registry.py:15-27 */
#define MMW_CFAR_CA 0
#define MMW_CFAR_OS 1
#define MMW_CFAR_GO 2
#define MMW_CFAR_SO 3

/* ---------------------------------------------------------------- lifecycle */
const char *mmw_version(void);
/* Bumped whenever an exported signature changes: a binding checks it at load (the argtypes of a ctypes binding are
 * hard-coded, so a library of another revision would reinterpret ints as device pointers). */
#define MMWGPU_ABI_VERSION 7
int mmw_abi_version(void);
const char *mmw_last_error(void);
int mmw_device_count(int *count);
/* Device name and gcnArchName into caller buffers (for fail-loud checks and reports). */
int mmw_device_info(int device, char *name, int name_len, char *arch, int arch_len,
                    int *num_cu, size_t *total_mem);
int mmw_ctx_create(mmw_ctx **out, int device);
int mmw_ctx_destroy(mmw_ctx *ctx);
int mmw_sync(mmw_ctx *ctx);

/* ---------------------------------------------------------------- memory */
int mmw_malloc(mmw_ctx *ctx, void **d_ptr, size_t bytes);
int mmw_free(mmw_ctx *ctx, void *d_ptr);
int mmw_memcpy_h2d(mmw_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int mmw_memcpy_d2h(mmw_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int mmw_memset(mmw_ctx *ctx, void *d_dst, int value, size_t bytes);

/* ---------------------------------------------------------------- host streaming
 * For frame loops whose cubes arrive on the host (the reference's scripts/test_vel_estimation.py:145-151): pinned staging
 * blocks, asynchronous copies on the compute queue or on a separate copy queue, and events to order the two, so that
 * chunk k + 1 is uploaded while chunk k is processed (batch.FramePipeline.stream).
 *   mmw_host_alloc / mmw_host_free   pinned host memory owned by the context
 *   mmw_memcpy_async                 to_host = 0: host -> device, 1: device -> host; queue = MMW_QUEUE_*; returns at once
 *   mmw_event_create / _destroy / _record(queue) / mmw_queue_wait_event(queue, event) / mmw_event_sync(event) */
#define MMW_QUEUE_COMPUTE 0
#define MMW_QUEUE_COPY    1
int mmw_host_alloc(mmw_ctx *ctx, void **h_ptr, size_t bytes);
int mmw_host_free(mmw_ctx *ctx, void *h_ptr);
int mmw_memcpy_async(mmw_ctx *ctx, void *dst, const void *src, size_t bytes, int to_host, int queue);
int mmw_event_create(mmw_ctx *ctx, void **event);
int mmw_event_destroy(mmw_ctx *ctx, void *event);
int mmw_event_record(mmw_ctx *ctx, void *event, int queue);
int mmw_queue_wait_event(mmw_ctx *ctx, int queue, void *event);
int mmw_event_sync(mmw_ctx *ctx, void *event);

/* ---------------------------------------------------------------- timing (HIP events on the ctx stream) */
int mmw_timer_start(mmw_ctx *ctx);
int mmw_timer_stop(mmw_ctx *ctx, float *elapsed_ms);   /* synchronises on the stop event */

/* ---------------------------------------------------------------- input staging
 * mmw_synth_cubes: fill d_cubes[n_frames][V][S][C] complex64 with the synthetic
 *   point-target + noise workload directly in HBM (counter-based RNG; integer-valued
 *   I/Q like SURVEY.md 8d).  Benchmark input only -- parity tests download these
 *   cubes and hand the SAME bytes to the oracle.
 * mmw_virtual_array_reformat: raw [F][num_rx][S][num_tx*loops] -> [F][num_rx*num_tx][S][loops]
 *   replaces VirtualArrayReformatter.process (processors/virtual_array_reformater.py:44-65). */
int mmw_synth_cubes(mmw_ctx *ctx, void *d_cubes, int n_frames, int V, int S, int C,
                    uint64_t seed0, int num_targets, float noise_sigma);
int mmw_virtual_array_reformat(mmw_ctx *ctx, const void *d_raw, void *d_virt, int n_frames,
                               int num_rx, int num_tx, int S, int loops);
/* mmw_virtual_array_reformat_i16: the same from int16 I/Q samples, raw [F][num_rx][S][num_tx*loops][2] (I, Q) ->
 *   complex64 [F][num_rx*num_tx][S][loops] (half the bytes over PCIe and HBM).  NO UPSTREAM ORACLE for this sample
 *   layout: the reference receives complex cubes from the cpsl_datasets reader, which is not part of its tree
 *   (SURVEY.md F3); the layout here is "the raw cube of mmw_virtual_array_reformat with int16 I/Q pairs". */
int mmw_virtual_array_reformat_i16(mmw_ctx *ctx, const void *d_raw_i16, void *d_virt, int n_frames,
                                   int num_rx, int num_tx, int S, int loops);

/* ---------------------------------------------------------------- FFT chain
 * mmw_range_doppler: d_out[F][V][S][C] c64 = fftshift_C( FFT_S FFT_C( hann(S) hann(C) x ) )
 *   replaces RangeDopplerProcessor.process (processors/range_doppler_resp.py:49-110) and
 *   RangeDopplerDetector._compute_range_doppler_response (range_doppler_detection/range_doppler_detector.py:62-80).
 *   If d_mag_f32 != NULL also writes |out| [F][V][S][C] float32 (return_magnitude=True path).
 * mmw_range_doppler_mag64: double-precision |RD| of ONE virtual antenna, d_mag[F][S][C] float64.
 *   This is the CFAR input plane (range_doppler_detector.py:78 uses rx 0 only); computed
 *   end-to-end in float64 so detection indices are bit-exact against the float64 reference.
 * mmw_angle_fft: d_out[F][A][S][C] c64 = fftshift_A FFT_A( zero-pad_{V->A}( hann(V) rd ) )
 *   last stage of RangeAngleProcessorDBSEnhanced.compute_3d_windowed_fft
 *   (processors/range_angle_resp_dbs_enhanced.py:175-196).  With MMW_ANGLE_MAGNITUDE the output is
 *   float32 |.| [F][A][S][C] instead (perform/process_dbs_enhanced :293).  Any 1 <= V <= A <= 4096; the shift is
 *   np.fft.fftshift's for odd A too (out[(k + A/2) mod A] = X[k]).  The window is np.hanning(V), whose end points are 0:
 *   with V = 2 (so at A = 2 with the window on) every output is exactly zero, as the reference's would be, and with
 *   V = 1 the window is [1]; MMW_ANGLE_NO_WINDOW is the way to a two-antenna spectrum.
 * mmw_chain3d: mmw_range_doppler followed by mmw_angle_fft, chunked so the RD intermediate
 *   stays cache-resident; d_rd may be NULL (internal scratch) or [F][V][S][C] to keep it.
 *   Replaces compute_3d_windowed_fft (:137-198) end to end. */
int mmw_range_doppler(mmw_ctx *ctx, const void *d_cubes, void *d_out, void *d_mag_f32,
                      int n_frames, int V, int S, int C);
int mmw_range_doppler_mag64(mmw_ctx *ctx, const void *d_cubes, double *d_mag,
                            int n_frames, int V, int S, int C, int rx_idx);
/* flags of mmw_angle_fft / mmw_chain3d (0 = complex64 output, Hann(V) window, fftshift over angle) */
#define MMW_ANGLE_MAGNITUDE 1   /* float32 |.| output                                                    */
#define MMW_ANGLE_NO_WINDOW 2   /* no antenna window (DopplerAzimuthProcessor on "ods" geometry)         */
#define MMW_ANGLE_NO_SHIFT  4   /* no fftshift over the angle axis (shift_angle=False)                   */
int mmw_angle_fft(mmw_ctx *ctx, const void *d_rd, void *d_out, int n_frames,
                  int V, int S, int C, int A, int flags);
int mmw_chain3d(mmw_ctx *ctx, const void *d_cubes, void *d_rd, void *d_out, int n_frames,
                int V, int S, int C, int A, int flags);
/* Raw-cube variants: d_raw[F][num_rx][S][num_tx * loops] c64 as the DCA1000 delivers it; the virtual-array
 *   de-interleave of VirtualArrayReformatter.process (virtual antenna tx * num_rx + rx = every num_tx-th chirp from
 *   tx, processors/virtual_array_reformater.py:53-63) is folded into the first kernel's loads, so
 *   mmw_range_doppler_raw == mmw_virtual_array_reformat + mmw_range_doppler and
 *   mmw_chain3d_raw == mmw_virtual_array_reformat + mmw_chain3d without the extra pass over HBM
 *   (V = num_rx * num_tx, C = loops; outputs as for the non-raw calls). */
int mmw_range_doppler_raw(mmw_ctx *ctx, const void *d_raw, void *d_out, int n_frames, int num_rx, int num_tx,
                          int S, int loops);
int mmw_chain3d_raw(mmw_ctx *ctx, const void *d_raw, void *d_rd, void *d_out, int n_frames, int num_rx, int num_tx,
                    int S, int loops, int A, int flags);
/* int16 (I, Q) raw cubes [F][num_rx][S][num_tx * loops][2]: conversion and de-interleave inside the first kernel's loads
 * (256 x 128 planes and every plane shape of the shipped cfgs; other shapes convert first), no complex64 cube in between.
 * NO UPSTREAM ORACLE for the sample layout (the reference's reader, cpsl_datasets, is not in its tree): defined as
 * mmw_virtual_array_reformat_i16 + the virtual-array entry point, and bit-identical to that. */
int mmw_range_doppler_raw_i16(mmw_ctx *ctx, const void *d_raw_i16, void *d_out, int n_frames, int num_rx, int num_tx,
                              int S, int loops);
int mmw_chain3d_raw_i16(mmw_ctx *ctx, const void *d_raw_i16, void *d_rd, void *d_out, int n_frames, int num_rx,
                        int num_tx, int S, int loops, int A, int flags);
/* mmw_dbs_gather: d_out[F][S][n_out] float32 = d_mag[F][h_ang_idx[i]][s][h_vel_idx[i]] -- the Doppler-beam-
 *   sharpening column pick of perform_dbs_sharpen (processors/range_angle_resp_dbs_enhanced.py:216-263); the
 *   nearest-bin index tables are computed by the host from its angle / velocity bin tables. */
int mmw_dbs_gather(mmw_ctx *ctx, const float *d_mag, const int *h_ang_idx, const int *h_vel_idx, float *d_out,
                   int n_frames, int A, int S, int C, int n_out);
/* mmw_dbs_sharpen: d_out[F][S][n_out] float32 = the Doppler-beam-sharpened range-azimuth image of every frame, each frame
 *   with index tables of its own (frames of a recording move at different velocities):
 *     rx = h_rx[n_rx] (n_rx == 0: all V antennas), n = len(rx), w = np.hanning(n),
 *     b  = (h_ang_idx[f][i] - A/2) mod A      the FFT bin behind the fftshifted angle index,
 *     k  = h_vel_idx[f][i]                    the fftshifted Doppler index, as mmw_range_doppler stores its cube,
 *     d_out[f][s][i] = | sum_j w[j] RD[f][rx[j]][s][k] exp(-2 pi i j b / A) |,   RD = mmw_range_doppler(d_cubes).
 *   This is |compute_3d_windowed_fft(cube[rx])|[h_ang_idx[f][i], s, h_vel_idx[f][i]] -- process_dbs_enhanced and
 *   perform_dbs_sharpen (processors/range_angle_resp_dbs_enhanced.py:216-263,265-300: antenna subset first, Hann over the
 *   subset, zero-pad to A) -- as a single-bin angle DFT per pixel: no [A][S][C] cube is allocated or written.  The tables
 *   are host arrays [F][n_out] (the nearest-bin argmins of :240-257, made by the caller from its bin tables).
 *   d_rd: NULL = the range-Doppler cubes pass through library scratch in chunks of frames, else [F][V][S][C] c64 to keep them.
 *   MMW_ERR_INVALID (nothing launched) names the frame and entry of a table value outside [0, A) / [0, C), an rx outside
 *   [0, V), n > 32, A < n, or n_frames * S * n_out beyond 2^31 - 1.  n_frames == 0 or n_out == 0: MMW_OK, nothing launched.
 *   Profile family "dbs_sharpen" (the range-Doppler pass counts under "rd"). */
int mmw_dbs_sharpen(mmw_ctx *ctx, const void *d_cubes, void *d_rd, const int32_t *h_ang_idx, const int32_t *h_vel_idx,
                    float *d_out, int n_frames, int V, int S, int C, int A, const int *h_rx, int n_rx, int n_out);
/* mmw_micro_doppler: d_out[F][C] float32 = the micro-Doppler row of every frame,
 *     d_out[f][c] = max_{row_lo <= r <= row_hi} | X_f[r][(c + C - C/2) mod C] |,   X_f = FFT_S FFT_C( d_cubes[f][rx_idx] ),
 *   no window, np.fft.fftshift's convention on the chirp axis (odd C included).  This is the column that
 *   MicroDopplerProcessor.process (processors/micro_doppler_resp.py:91-114) rolls into its spectrogram: |fftshift(fft2(x[rx]))|,
 *   the rows of the range window, np.max over them.  Only antenna rx_idx's [S][C] slab of a frame is read, only the rows of the
 *   window are computed (a partial DFT over fast time, direct DFTs over slow time, float32), and nothing but the C floats of a
 *   frame is written.  Any S, C >= 1 up to 3444 chirps (MMW_ERR_UNSUPPORTED beyond: the rows in flight live in the LDS).
 *   Range: the magnitude is sqrt(re^2 + im^2) in float32, not hypot.  Scaling a slab by 2^e scales its row by 2^e bit for bit, and
 *   every value lies within ulps(S, C) 2^-24 of L1 = sum |x[s][c]| from the exact one (tests/partial_dft_cases.py counts ulps),
 *   for as long as every partial sum, im^2 and re^2 + im^2 of the frame are normal, finite float32 numbers; L1 < 2^63 keeps them
 *   finite, and an output below 2^-63 may have lost its precision or be 0.  A NaN anywhere in the slab (either sign) makes the
 *   frame's whole row NaN, an infinity leaves no finite value in it, an all-zero slab gives +0.0; other frames and the other
 *   antennas are not touched by either.
 *   MMW_ERR_INVALID (nothing launched, d_out untouched): a null pointer, n_frames < 0, rx_idx outside [0, V), row_lo > row_hi,
 *   a row outside [0, S).  n_frames == 0: MMW_OK, nothing launched.  Profile family "micro_doppler". */
int mmw_micro_doppler(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C, int rx_idx, int row_lo,
                      int row_hi);
/* mmw_sar_slices: per frame f one window of the un-windowed range-Doppler plane of antenna rx_idx, complex64, packed:
 *     block f = d_out + h_off[f], row-major [row_hi - row_lo][col_hi - col_lo],
 *     block_f[r - row_lo][c - col_lo] = sum_s sum_j x_f[rx_idx][s][j] exp(-2 pi i (r s / S + j k / C)),   k = (c + C - C/2) mod C,
 *   i.e. np.fft.fftshift(np.fft.fft2(x), axes=1)[row_lo:row_hi, col_lo:col_hi] (odd C included): what StripMapSARProcessor.process
 *   (processors/strip_map_SAR_processor.py:160-194) keeps of the plane -- [valid_ranges_slice, valid_angles_slice], the columns
 *   a function of that frame's platform speed (:108-158), hence a window per frame and a ragged output.  h_win[F][4] holds
 *   (row_lo, row_hi, col_lo, col_hi), half open; h_off[F + 1] the blocks' first elements in complex64 units, h_off[F] the total.
 *   Both are host arrays, free again when the call returns.  Only antenna rx_idx's [S][C] slab of a frame is read, only the listed
 *   rows and columns are computed (a partial DFT over fast time, direct DFTs over slow time, float32), and nothing but the blocks
 *   is written; a frame whose window is empty in either axis writes nothing.  Any S >= 1 and any C <= 3444 -- the shapes
 *   mmw_micro_doppler serves (MMW_ERR_UNSUPPORTED beyond: the rows in flight live in the LDS; the shape is judged before the
 *   windows, so also when every window is empty, where a served shape returns MMW_OK with nothing launched).  The grid is capped at 4096
 *   workgroups; with more frames a workgroup walks frames f, f + 4096, ...
 *   Range: the blocks are complex and nothing is squared, so the same bound (every element within ulps(S, C) 2^-24 L1 of the exact
 *   one) and the bit-for-bit scaling by 2^e hold on the wider interval on which every partial sum is a normal, finite float32
 *   number; L1 < 2^127 keeps them finite.  A NaN in the slab makes every element of the frame's block NaN, an infinity leaves
 *   none finite, an all-zero slab gives +0.0 in both parts; other frames are not touched.
 *   MMW_ERR_INVALID (nothing launched, d_out untouched): a null pointer, n_frames < 0, rx_idx outside [0, V), a window reversed
 *   or outside [0, S] x [0, C], h_off[0] != 0, h_off[f + 1] - h_off[f] different from the window's area.  n_frames == 0: MMW_OK,
 *   nothing launched.  Profile family "sar_slices". */
int mmw_sar_slices(mmw_ctx *ctx, const void *d_cubes, int n_frames, int V, int S, int C, int rx_idx,
                   const int32_t *h_win /* [F][4]: row_lo,row_hi,col_lo,col_hi, half open */,
                   const int64_t *h_off /* [F+1], in complex64 elements */, void *d_out);
/* mmw_range_detect: RangeDetector.process (processors/range_detector.py:59-83) for F frames in one call, no host round trip:
 *   the float64 range profile of chirp chirp_idx (mmw_range_profile_f64's values; into d_profile[F][S], or library scratch when
 *   NULL), the 1-D CFAR of mmw_cfar1d on every profile (same arguments, thresholds and decisions bit-identical to it; the
 *   thresholds into d_thr[F][S] unless NULL) and the cells above their threshold in ascending order in d_dets[F][cap], their
 *   number in d_counts[F] -- exact also when a frame overflows cap, as in mmw_compact2d; entries past the count are not written.
 *   S as far as mmw_range_profile_f64 serves it (and never beyond 49152: MMW_ERR_UNSUPPORTED), n_frames <= 65535.  MMW_ERR_INVALID (nothing launched): a null d_cubes / d_dets /
 *   d_counts / ctx, n_frames outside [0, 65535], a non-positive shape, chirp_idx outside [-C, C), cap < 0, CFAR arguments
 *   mmw_cfar1d refuses.  n_frames == 0: MMW_OK.  Profile family "range_detect" (the profile pass counts under its own). */
int mmw_range_detect(mmw_ctx *ctx, const void *d_cubes, int n_frames, int V, int S, int C, int chirp_idx, int kind, int num_train,
                     int num_guard, double scale, int k_rank, double *d_profile, double *d_thr, int32_t *d_dets,
                     int32_t *d_counts, int cap);
/* mmw_synth_array: the synthetic-array images of n_out frames of a resident batch, their windows read in place,
 *     d_out[i] = FFT_S( hann(S) . ( X_i[S][E] x W_i[E][T] ) ),   W_i[e][t] = hamming(E)[e] exp(j 2 pi d_t . p_{i,e} / lambda),
 *   Cv = ceil(C / k), E = H Cv, element e = (h, j) of X_i = d_cubes[h_frames[i] - H + 1 + h][v][s][j k]: the last H frames of
 *   every k-th chirp of virtual antenna v, oldest frame first -- SyntheticArrayBeamformerProcessor's history_acd_cube_valid_chirps
 *   (processors/simple_synthetic_array_beamformer_processor_multiFrame.py:818-872) without the [n_out][S][E] copy: this is
 *   mmw_bartlett with its operand gathered from d_cubes [n_resident][V][S][C] c64 inside the kernels.  A window frame with a
 *   negative index is all zeros and is never read; the Hamming taper and the geometry still count its elements.
 *   h_frames [n_out] host int32, strictly ascending, each in [0, n_resident); h_P [n_out][3][E] host float64 (element positions
 *   of every window); h_dirs [3][T] host float64; d_out [n_out][S][T] c64.  The host arrays are free again when the call returns.
 *   MMW_ERR_INVALID (nothing enqueued, d_out untouched): a null pointer, v outside [0, V), k < 1, H < 1, T < 1, lambda_m <= 0,
 *   n_out outside [0, 65535], h_frames unsorted / repeated / out of range.  n_out == 0: MMW_OK, nothing launched.
 *   The MMW_BARTLETT_* options select the kernels as they do for mmw_bartlett.  Profile family "synth_array".
 * mmw_diag_synth_array_window: the window arithmetic behind it, host only (no device, no context): the run of n elements from e0
 *   of output frame `frame` cut at the frame boundaries -- h_segs[4 i ..] = (window slot, resident frame or negative, first chirp
 *   index j, elements) for up to cap segments; info[0] = segments, [1] = first resident frame read (-1: none), [2] = the run may be
 *   read with 16-byte loads, [3] = the tile kernels' 16-byte path is legal for runs of n at this (C, k, H). */
int mmw_synth_array(mmw_ctx *ctx, const void *d_cubes, int n_resident, int V, int S, int C, int v, int k, int H,
                    const int32_t *h_frames, int n_out, const double *h_P, const double *h_dirs, int T, double lambda_m, void *d_out);
int mmw_diag_synth_array_window(int C, int k, int H, int frame, int e0, int n, int32_t *h_segs, int cap, int32_t info[4]);
/* mmw_synth_array_calibrate: mmw_synth_array followed by n_iters rounds of self-calibration against targets of opportunity and a
 *   contraction with the corrected geometry (mmw_synth_calib.h), all enqueued without a host synchronisation.
 *   Arguments as mmw_synth_array with T = n_az n_el directions laid out [3][n_az][n_el]; picks use elevation index 0.
 *   d_out [n_out][S][T] c64: the last image computed for every frame; d_Pcal [n_out][3][E] f64: the calibrated geometry (the
 *   uncalibrated one where the loop stopped for lack of three targets, and for flagged frames); d_status [n_out] int32: the
 *   iterations that applied a correction (0 .. n_iters), or -1: a decision fell inside the rounding band of its inputs, a phase
 *   step lies within its error of +-pi, or the 3 x 2 system has a condition number above 1e6 -- the caller calibrates that frame on
 *   the host; d_targets [n_out][3][2] int32: (range row, azimuth bin) of the last iteration that found three targets; -1 where none did, and for every flagged frame.
 *   Unlike the reference (IndexError), fewer than three range peaks, and a non-finite avg (a window slot before the buffer is
 *   all zeros: log10(0)), count as "no suitable targets": status 0.
 *   MMW_ERR_INVALID (nothing enqueued, outputs untouched): what mmw_synth_array refuses, a null output, n_iters outside [1, 8],
 *   n_az or n_el < 1 or n_az n_el beyond int32.  MMW_ERR_UNSUPPORTED: S > 3584 (avg and its error bound live in the LDS).  n_out == 0: MMW_OK.
 *   Option MMW_SYNTH_CALIB_FLAG_ALL=1 flags every frame.  Profile family "synth_calib" (inside it: "synth_calib_spectra",
 *   "synth_calib_frame", and the contractions as "synth_array").
 * mmw_diag_synth_array_calib_host: steps 3-6 of one window on host pointers (no device, no context), the decision and solve code of
 *   the kernels: h_avg [S] with error bounds h_avg_err [S] (null: exact), h_mag [S][n_az] image magnitudes at elevation 0 known to
 *   +-mag_band, h_Fq [S][E] complex128 (the three picked rows are read), h_l1 [E] L1 norms of the columns for the phase error bound
 *   (null: exact), h_P [3][E], h_dirs [3][n_az n_el] -> h_Pcal [3][E], h_targets [3][2], info = {1 applied / 0 no suitable targets /
 *   -1 flagged, reasons (1 range, 2 azimuth, 4 phase wrap, 8 condition), 3 when three range peaks were found, condition > 1e6}.
 *   An ill-conditioned system is flagged and still solved (minimum norm). */
int mmw_synth_array_calibrate(mmw_ctx *ctx, const void *d_cubes, int n_resident, int V, int S, int C, int v, int k, int H,
                              const int32_t *h_frames, int n_out, const double *h_P, const double *h_dirs, int n_az, int n_el,
                              double lambda_m, int n_iters, void *d_out, double *d_Pcal, int32_t *d_status, int32_t *d_targets);
int mmw_diag_synth_array_calib_host(const double *h_avg, const double *h_avg_err, int S, const double *h_mag, double mag_band, int n_az,
                                    int n_el, const double *h_Fq, const double *h_l1, int E, const double *h_P, const double *h_dirs,
                                    double lambda_m, double *h_Pcal, int32_t *h_targets, int32_t info[4]);
/* mmw_synth_array_pattern: the beam patterns (array factors) of n synthetic-array geometries, no taper and no data (DESIGN.md 4.26,
 *   mmw_synth_pattern.h; SyntheticArrayBeamformerProcessor.compute_synthetic_array_pattern,
 *   processors/simple_synthetic_array_beamformer_processor_multiFrame.py:615-670):
 *     AF_i[t] = sum_e exp(j 2 pi d_t . p_{i,e} / lambda) in float64,  a_i[t] = float32(|AF_i[t]|),  pattern_i[t] = a_i[t] / max_t a_i[t]
 *   with the division and the maximum in float32.  d_P [n][3][E] DEVICE float64 -- the layout of mmw_synth_array's h_P, and of the
 *   d_Pcal mmw_synth_array_calibrate leaves behind, which is read in place; h_dirs [3][T] HOST float64, free again when the call
 *   returns; d_pattern [n][T] float32; d_af [n][T] complex128, the un-normalised AF, or NULL.  The phase is reduced in cycles before
 *   the sine and cosine and the summation order is fixed: a call repeats bit for bit.  A frame with a non-finite coordinate gives
 *   an all-NaN pattern (as numpy), the other frames are unaffected; 0 / 0 is what IEEE makes it.  The normalisation is enqueued
 *   behind the magnitudes, no host synchronisation.
 *   MMW_ERR_INVALID (nothing enqueued, outputs untouched): a null ctx / d_P / h_dirs / d_pattern, n < 0, E < 1, T < 1, lambda_m
 *   not finite or <= 0, n T or 3 n E beyond int32.  n == 0: MMW_OK, nothing launched.  Profile family "synth_pattern".
 * mmw_diag_synth_array_pattern_host: the same accumulation (one implementation, mmw_synth_pattern.h) on host pointers; no context,
 *   no device. */
int mmw_synth_array_pattern(mmw_ctx *ctx, const double *d_P, int n, int E, const double *h_dirs, int T, double lambda_m,
                            float *d_pattern, void *d_af);
int mmw_diag_synth_array_pattern_host(const double *h_P, int n, int E, const double *h_dirs, int T, double lambda_m,
                                      float *h_pattern, void *h_af);
/* mmw_mean_over_range: d_out[F][C][A] float32 = mean over range rows [s_lo, s_hi) of d_mag[F][A][S][C];
 *   with mmw_chain3d(flags | MAGNITUDE) this is DopplerAzimuthProcessor.process, coarse path
 *   (processors/doppler_azimuth_resp.py:84-128,296-334,419-491): range FFT -> range-window mask ->
 *   2-D FFT over (chirp, antenna) -> |.| -> mean over the kept range bins. */
int mmw_mean_over_range(mmw_ctx *ctx, const float *d_mag, float *d_out, int n_frames,
                        int A, int S, int C, int s_lo, int s_hi);
/* mmw_doppler_azimuth: d_out[F][C][A] float32 = mean over range rows [s_lo, s_hi) of
 *   | fftshift_A FFT_A( pad_{V->A}( hann(V) RD[v][s][c] ) ) |, RD = the windowed range-Doppler spectrum of mmw_range_doppler:
 *   DopplerAzimuthProcessor.process, coarse path (processors/doppler_azimuth_resp.py:84-128,296-334,419-491) in one
 *   call; the [A][S][C] magnitude cube is never written (the angle FFT, |.| and the range mean are one kernel).
 *   flags: MMW_ANGLE_NO_WINDOW, MMW_ANGLE_NO_SHIFT.  Same result as mmw_chain3d(MAGNITUDE) + mmw_mean_over_range. */
int mmw_doppler_azimuth(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C, int A,
                        int s_lo, int s_hi, int flags);
/* mmw_doppler_azimuth_zoom: d_out[F][M][A] float32 = mean over range rows [s_lo, s_hi) of
 *   | fftshift_A FFT_A( pad_{V->A}( hann(V)[v] sum_{c < n_used} R[v][s][c] exp(-j 2 pi c h_freq[k]) ) ) |,
 *   R = FFT_S( hann(S) hann(C) x ), h_freq[M] in cycles per chirp (host array; NaN = a bin the reference fills
 *   with zeros).  This is DopplerAzimuthProcessor.process(use_precise_fft=True)
 *   (processors/doppler_azimuth_resp.py:130-163,208-294,477-489), whose two scipy.signal.ZoomFFT calls over the
 *   chirp axis evaluate exactly these sums; the caller derives h_freq from the velocity range (:148-155,254-283).
 *   flags: MMW_ANGLE_NO_WINDOW, MMW_ANGLE_NO_SHIFT. */
int mmw_doppler_azimuth_zoom(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C, int A,
                             int s_lo, int s_hi, int n_used, const double *h_freq, int M, int flags);
/* mmw_doppler_azimuth_batch: the coarse Doppler-azimuth maps of n_sets antenna subsets of every frame of a resident batch, each
 * frame with a range window of its own:
 *     d_out[k][f][c][a] (float32 [n_sets][F][C][A]) = mean over rows s in [h_rows[f][0], h_rows[f][1]) of
 *         | fftshift_A FFT_A( pad_{n->A}( hann(n)[j] RD_f[h_rx[k][j]][s][c] ) ) |,   RD = mmw_range_doppler's windowed spectrum,
 *   i.e. DopplerAzimuthProcessor.process(cube_f[rx_k], range_window_f, shift_angle_k) before the valid-angle mask: the subset is
 *   taken first and the Hann window spans the subset.  d_cubes [F][V][S][C] c64 as resident.  h_rx: host int32 [n_sets][n_rx];
 *   n_rx == 0 (then n_sets == 1, V <= 16): all V antennas.  h_set_flags[n_sets]: MMW_ANGLE_NO_SHIFT per set.  flags:
 *   MMW_ANGLE_NO_WINDOW for all sets.  h_rows: host int32 [F][2].  A frame with lo == hi gets NaN (np.mean over an empty axis).
 *   The range-Doppler pass runs once per chunk of frames for all sets (profile family "rd"); the angle FFT, |.| and the range
 *   mean are one kernel reading its n <= 16 inputs through the antenna list (family "dopaz_batch"); no [A][S][C] cube is written.
 *   Intermediates stay within MMW_DOPAZ_CHUNK_MB (default 1024) per pass; a frame's result does not depend on the chunking.
 *   MMW_ERR_INVALID (nothing launched, d_out untouched; the text names the frame / set / entry): a null pointer, n_frames < 0,
 *   n_sets < 1, n_rx outside [0, 16], an antenna outside [0, V) or repeated within a set, a row interval outside
 *   0 <= lo <= hi <= S, unknown flag bits, n_sets * F * C * A beyond 2^31 - 1.  MMW_ERR_UNSUPPORTED: A != 64 (the single-frame
 *   entries take other sizes).  n_frames == 0: MMW_OK, nothing launched. */
int mmw_doppler_azimuth_batch(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C, int A,
                              const int32_t *h_rx, int n_sets, int n_rx, const int32_t *h_set_flags, const int32_t *h_rows, int flags);
/* mmw_doppler_azimuth_zoom_batch: the precise (zoom) maps of the same batch, each frame with a frequency list of its own:
 *     d_out[k][f][m][a] (float32 [n_sets][F][M][A]) = mmw_doppler_azimuth_zoom's formula on cube_f[rx_k] with rows h_rows[f] and
 *   the list h_freq[f][0..M) (host float64 [F][M], cycles per chirp).  NaN marks a bin the reference fills with zeros and pads a
 *   frame whose list is shorter than M: those rows of d_out are exactly 0.  n_used in [1, C] chirps enter the transform.
 *   The range FFT runs once per chunk for all sets; the zoom transform is a direct sum on the rows of each frame's window and the
 *   antennas some set uses, twiddles from the float64 phase (no per-list plan).  Profile family "dopaz_zoom_batch" (its phases
 *   also under "dopaz_zoom_range", "dopaz_zoom_rows", "dopaz_zoom_mean").  Limits as mmw_doppler_azimuth_batch, with
 *   n_sets * F * max(C, M) * A <= 2^31 - 1 and n_used outside [1, C] refused; more than 320 chirps: MMW_ERR_UNSUPPORTED. */
int mmw_doppler_azimuth_zoom_batch(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C, int A,
                                   const int32_t *h_rx, int n_sets, int n_rx, const int32_t *h_set_flags, const int32_t *h_rows, int flags,
                                   int n_used, const double *h_freq, int M);
/* mmw_doppler_azimuth_peaks: DopplerAzimuthProcessor.detect_peaks_rows / detect_peak_zero_az on the maps the two batch entries
 *   leave in HBM (or on any device buffer of that layout), for every frame and every group of sets:
 *     d_maps float32 [n_sets][F][n_rows][A];  h_groups host int32 [G][2]: the two sets whose maps are averaged as the reference's
 *     (resp_1 + resp_2) / 2, or (set, -1) for one set;  h_m host int32 [F]: the rows of each frame (NULL: n_rows);  the valid
 *     angle columns [a_lo, a_hi) and the zero-azimuth column a_zero among them.
 *     d_row_peak int32 [G][F][n_rows]: the column, relative to a_lo, of the row's strongest local maximum with at least
 *     prominence_dB of prominence;  d_zero int32 [G][F]: the row of the strongest local maximum down column a_zero.
 *     -1: no peak (rows >= m[f] as well);  -2: undecided.
 *   The rule is scipy.signal.find_peaks' on the map in dB, floored min_threshold_dB below the frame's maximum, restated in the
 *   linear domain in float64 (no log10 on the device).  A comparison of two map-derived quantities is decided only when they
 *   are bit-equal or differ by more than the relative MMW_DOPAZ_PEAK_BAND (a quantity against a product with a dB ratio: only
 *   when they differ by more, unless the ratio is exactly 1); otherwise the line is -2, and so is every line of a frame whose
 *   m[f] x [a_lo, a_hi) cells hold a NaN or an Inf: the host picks those frames with the dB rule.  Profile family "dopaz_peaks".
 *   MMW_ERR_INVALID (nothing launched, outputs untouched; the text names what was refused): a null pointer (h_m excepted), a
 *   negative count, a group index outside [0, n_sets) or a group naming one set twice, m[f] outside [0, n_rows], a column
 *   interval not 0 <= a_lo < a_hi <= A, a_zero outside [a_lo, a_hi), a dB parameter negative or not finite, element counts
 *   beyond 2^31 - 1.  MMW_ERR_UNSUPPORTED: A != 64.  F == 0 or G == 0: MMW_OK, nothing launched.
 * mmw_diag_doppler_azimuth_peaks_host: the same rule (one implementation, mmw_dopaz_peaks.h) on host pointers; no context, no
 *   device. */
#define MMW_DOPAZ_PEAK_BAND 1e-10
int mmw_doppler_azimuth_peaks(mmw_ctx *ctx, const float *d_maps, int n_sets, int F, int n_rows, int A, const int32_t *h_groups, int G,
                              const int32_t *h_m, int a_lo, int a_hi, int a_zero, double min_threshold_dB, double prominence_dB,
                              int32_t *d_row_peak, int32_t *d_zero);
int mmw_diag_doppler_azimuth_peaks_host(const float *h_maps, int n_sets, int F, int n_rows, int A, const int32_t *h_groups, int G,
                                        const int32_t *h_m, int a_lo, int a_hi, int a_zero, double min_threshold_dB,
                                        double prominence_dB, int32_t *h_row_peak, int32_t *h_zero);
/* mmw_doppler_azimuth_ransac: the regression stage of the Doppler-azimuth velocity estimator (processors/velocity_estimator.py:
 *   estimate_ego_vx_velocity :640-661, lsq_fit_ego_vy_ransac :346-506) on the index tables mmw_doppler_azimuth_peaks leaves in
 *   HBM, one fit per (group, frame), nothing downloaded:
 *     d_row_peak int32 [G][F][n_rows], d_zero int32 [G][F] (-1: none, -2: undecided);  h_m host int32 [F]: the rows of each
 *     frame (NULL: n_rows), rows >= m[f] are absent;  d_vel float64: one table [vel_len] for all frames (vel_per_frame == 0) or
 *     [F][vel_len] (the precise mode's zoomed_vel_bins), vel_len >= n_rows;  d_cos, d_sin, d_theta float64 [n_cols]: np.cos,
 *     np.sin of the valid angle bins and the bins themselves;  d_subsets int32 [n_tab][20][10]: row N - 10 holds the subsets
 *     scikit-learn draws for N points (ransac_tables.subset_table(N)), n_tab >= n_rows - 9;  d_trials int32 [trials_len]: the
 *     trial caps of N points (ransac_tables.trials_table(N), N + 1 entries) one behind the other from N = 10 to 9 + n_tab.
 *     vx = -1 * (v_az + v_el) / 2.0, -1 * v or 0.0 from the zero-azimuth entries of groups g_az and g_el (g_el == -1: no elevation
 *     group), in NumPy's operation order: bit-equal.  The peak list of (g, f) are its rows with an entry >= 0, in row order, N of
 *     them.  vx >= MMW_DOPAZ_VX_BRANCH: y = (-1 * v) - (vx * cos), H = sin, threshold thr_standard, vy = coef, R^2 of the refit on
 *     its inliers (0.0 with at most 3);  else y = theta, H = v - vx, threshold thr_small_vx, vy = -1 / a (0 for a == 0), R^2
 *     without the inlier gate.  The fit is RANSACRegressor(LinearRegression(fit_intercept=False), min_samples=10, max_trials=20,
 *     random_state=42) of scikit-learn 1.7.2, walked in its order.
 *     d_out float64 [G][F][4] = (vx, vy, R^2, inlier share);  d_flags int32 [G][F]: MMW_DOPAZ_FLAG_* bits in the low byte, the
 *     status MMW_DOPAZ_STATUS_* at MMW_DOPAZ_STATUS_SHIFT, the inlier count at MMW_DOPAZ_INLIERS_SHIFT.  STATUS_EMPTY: N == 0 (the
 *     caller keeps the previous frame's values);  STATUS_FAILED: N < 10 or no accepted trial (the class's ValueError path), row
 *     (vx, 0, 0, 0).  A decision rounding could turn against scikit-learn's SVD solve sets a flag bit and zeroes the row: the
 *     caller refits that pair on the host.  mode MMW_DOPAZ_RANSAC_VX_ONLY: only vx (x_measurement_only).
 *   One wavefront per (group, frame), four to a workgroup; profile family "dopaz_ransac".
 *   MMW_ERR_INVALID (nothing launched, outputs untouched; the text names what was refused): a null pointer (h_m excepted), a
 *   negative count, g_az outside [0, G) or g_el outside [-1, G), m[f] outside [0, n_rows], vel_len < n_rows, n_cols < 1, tables
 *   that do not serve n_rows (n_tab, trials_len), a threshold that is not finite, element counts beyond 2^31 - 1.
 *   MMW_ERR_UNSUPPORTED: n_rows > MMW_DOPAZ_RANSAC_MAX_ROWS.  F == 0 or G == 0: MMW_OK, nothing launched.
 * mmw_diag_doppler_azimuth_ransac_host: the same rule (one implementation, mmw_dopaz_velocity.h, the 64 lanes as a loop) on host
 *   pointers; no context, no device.  Rows and flags are bit-identical to the kernel's. */
#define MMW_DOPAZ_VX_BRANCH 0.1
#define MMW_DOPAZ_RANSAC_MAX_ROWS 512
#define MMW_DOPAZ_RANSAC_VX_ONLY 1
#define MMW_DOPAZ_FLAG_RESIDUAL 1    /* a residual within the band of the threshold in a trial */
#define MMW_DOPAZ_FLAG_SCORE_TIE 2   /* equal inlier counts, scores within the band, different inlier sets */
#define MMW_DOPAZ_FLAG_R2 4          /* R^2 within the band of min_R2, or ill-defined */
#define MMW_DOPAZ_FLAG_SHARE 8       /* the inlier share at min_inlier_share */
#define MMW_DOPAZ_FLAG_A_ZERO 16     /* the small-vx coefficient within the band of 0 */
#define MMW_DOPAZ_FLAG_NONFINITE 32  /* a non-finite table entry, or sums beyond the trusted range */
#define MMW_DOPAZ_FLAG_UNDECIDED 64  /* a -2 among the pair's inputs */
#define MMW_DOPAZ_FLAG_TABLES 128    /* an entry that is no index of its table (caller error; nothing computed) */
#define MMW_DOPAZ_FLAG_MASK 0xff
#define MMW_DOPAZ_STATUS_SHIFT 8
#define MMW_DOPAZ_STATUS_OK 0
#define MMW_DOPAZ_STATUS_EMPTY 1
#define MMW_DOPAZ_STATUS_FAILED 2
#define MMW_DOPAZ_STATUS_MASK 3
#define MMW_DOPAZ_INLIERS_SHIFT 16
int mmw_doppler_azimuth_ransac(mmw_ctx *ctx, const int32_t *d_row_peak, const int32_t *d_zero, int G, int F, int n_rows,
                               const int32_t *h_m, const double *d_vel, int vel_len, int vel_per_frame, const double *d_cos,
                               const double *d_sin, const double *d_theta, int n_cols, const int32_t *d_subsets,
                               const int32_t *d_trials, int n_tab, int trials_len, int g_az, int g_el, int mode,
                               double thr_standard, double thr_small_vx, double min_R2, double min_inlier_share, double *d_out,
                               int32_t *d_flags);
int mmw_diag_doppler_azimuth_ransac_host(const int32_t *h_row_peak, const int32_t *h_zero, int G, int F, int n_rows,
                                         const int32_t *h_m, const double *h_vel, int vel_len, int vel_per_frame,
                                         const double *h_cos, const double *h_sin, const double *h_theta, int n_cols,
                                         const int32_t *h_subsets, const int32_t *h_trials, int n_tab, int trials_len, int g_az,
                                         int g_el, int mode, double thr_standard, double thr_small_vx, double min_R2,
                                         double min_inlier_share, double *h_out, int32_t *h_flags);

/* mmw_range_profile: d_out[F][S] float32 = mean_rx | FFT_S( hann(S) x[:, :, chirp] ) |
 *   replaces RangeProcessor.coarse_fft (processors/range_resp.py:32-57).
 * mmw_range_angle: d_out[F][S][A] float32 = | fftshift_A fft2( pad_A( (win) x[rx, :, chirp].T ) ) |
 *   replaces RangeAngleProcessor.process (processors/range_angle_resp.py:55-122); the window is
 *   applied over ALL V antennas before the subset h_rx[n_rx] is taken (:96-101); n_rx == 0 = all. */
int mmw_range_profile(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames,
                      int V, int S, int C, int chirp_idx);
/* float64 variant feeding the 1-D range CFAR of RangeDopplerDetectorSequential
 * (processors/range_doppler_detection/range_doppler_detector_sequential.py:84-91). */
int mmw_range_profile_f64(mmw_ctx *ctx, const void *d_cubes, double *d_out, int n_frames,
                          int V, int S, int C, int chirp_idx);
/* mmw_range_zoom: d_out[F][m] float32 = mean_rx | sum_n hann(S)[n] x[rx][n][chirp] exp(-j 2 pi n (f0 + k df)) |,
 *   k = 0..m-1, frequencies in cycles per sample: the zoomed range profile of RangeProcessor.zoom_fft
 *   (processors/range_resp.py:59-102), which the reference evaluates with scipy.signal.ZoomFFT. */
int mmw_range_zoom(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C,
                   int chirp_idx, int m, double f0_cycles_per_sample, double df_cycles_per_sample);
int mmw_range_angle(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames,
                    int V, int S, int C, int A, int chirp_idx, const int *h_rx, int n_rx,
                    int perform_windowing);

/* ---------------------------------------------------------------- CFAR detectors (float64, like the reference)
 * mmw_cfar2d: thresholds/noise [F][R][D] float64 and det mask [F][R][D] uint8 for
 *   BaseCFAR2D.detect + Ca/OsCFAR2D._compute_thresholds (detectors/base.py:208-230,
 *   ca_cfar.py:85-155, os_cfar.py:134-195).  CA: scale = alpha = N(pfa^(-1/N)-1) computed by the
 *   caller (base.py:281-293), k_rank ignored.  OS: scale = alpha, k_rank 1-based (os_cfar.py:131-132).
 *   Valid region only; elsewhere threshold = +inf, noise = 0; decision X > T strict.
 *   d_thr / d_noise may be NULL when only the mask is wanted.
 * mmw_cfar1d: same for Ca/Os/Go/SoCFAR1D (ca_cfar.py:11-77, os_cfar.py:29-86, go_so_cfar.py:11-123)
 *   over n_rows independent rows of length L.
 * mmw_compact2d: ordered (row-major, == np.where, base.py:229-230) compaction of the mask into
 *   d_dets[F][cap][2] int32 (row, col) and d_counts[F] int32.  Counts are exact even when
 *   a frame overflows cap (status MMW_ERR_TRUNCATED is reported by mmw_detect_* wrappers). */
int mmw_cfar2d(mmw_ctx *ctx, const double *d_X, double *d_thr, double *d_noise, uint8_t *d_mask,
               int n_frames, int R, int D, int kind, int train_r, int train_d,
               int guard_r, int guard_d, double scale, int k_rank);
int mmw_cfar1d(mmw_ctx *ctx, const double *d_x, double *d_thr, double *d_noise, uint8_t *d_mask,
               int n_rows, int L, int kind, int num_train, int num_guard, double scale, int k_rank);
int mmw_compact2d(mmw_ctx *ctx, const uint8_t *d_mask, int32_t *d_dets, int32_t *d_counts,
                  int n_frames, int R, int D, int cap);

/* Batched RangeDopplerGroundDetector (range_doppler_detection/range_doppler_ground_detector.py:72-127 per frame; the
 * Altimeter's state -- one scalar gate -- stays on the host, everything it gates is computed here for F frames at once).
 * mmw_ground_candidates: d_profile[F][S] float64 = the chirp-0 range profile of mmw_range_profile_f64, then
 *   RangeProcessor.find_peaks(20 log10(profile), bins, max_peaks=3) (processors/altimeter.py:79-96 -> range_resp.py:104-149,
 *   scipy.signal.find_peaks(prominence=6), `>= max - 20`, strongest first) on the device: d_cand[F][3] = d_bins[peak],
 *   d_counts[F] = number of candidates, or -1 when the frame holds a decision within the picker's rounding band (the host
 *   then runs find_peaks on d_profile[f]).  S <= 3072.
 * mmw_ground_zoom_candidates: for every candidate c < d_counts[f] of every frame, Altimeter._look_zoom's window
 *   [max(1e-6, c - half_width_m), min(hi_cap_m, c + half_width_m)] (hi_cap_m = max(range_bins) - 1e-6) on S bins:
 *   d_spec[F][3][S] float64 = mean over antennas of |DFT| of hann(S) * chirp 0 at those ranges (RangeProcessor.zoom_fft,
 *   range_resp.py:59-102, which the reference evaluates with scipy's float64 ZoomFFT; fs = 1 / range_res_m), then the same
 *   picker with max_peaks=2: d_zcand[F][3][2] = np.linspace(lo, hi, S)[peak], d_zcounts[F][3] (0 past d_counts[f], -1:
 *   flagged, the host runs find_peaks on d_spec[f][c]).  S <= 2048.
 * mmw_cfar1d_gated: the 1-D CFAR of mmw_cfar1d (bit-identical decisions) along Doppler on the rows d_gate[f] = (near, far),
 *   both included, of each frame's d_mag64[F][R][D] (the reference's per-row vel_detector.detect, :110-120), then the ordered
 *   compaction of mmw_compact2d into d_dets[F][cap][2] / d_counts[F] (exact counts on overflow).  d_mask[F][R][D] is work
 *   space.  Context option MMW_GROUND_FLAG_ALL = 1: both candidate entries flag every frame / window (tests of the host path).
 * mmw_cfar1d_rows: mmw_cfar1d_gated with the rows of frame f named by the ascending list d_rows[F][R] int32, first d_nrows[f]
 *   entries (the lists of mmw_seq_rows; a length below 0 counts as 0, one above R as R; an entry outside [0, R) names no row),
 *   in place of a gate: the second half of mmw_seq_detect_plane on a caller's plane.  Every cell of d_mask is written, 0 in
 *   the rows that are not listed.
 * mmw_diag_ground_pick: the picker of mmw_ground_candidates alone on a caller's d_profile[n_rows][S] float64 (linear values, one
 *   workgroup per row), max_peaks 2 or 3: d_cand[n_rows][3] = d_bins[peak] in its first d_counts[row] slots (the others are not
 *   written), d_counts[n_rows] as above, -1 included.  Refusals as mmw_ground_candidates (S >= 3, S <= 3072, n_rows <= 65535,
 *   MMW_ERR_INVALID, nothing launched); honours MMW_GROUND_FLAG_ALL.  For tests of the picker's decisions. */
int mmw_ground_candidates(mmw_ctx *ctx, const void *d_cubes, const double *d_bins, double *d_profile, double *d_cand,
                          int32_t *d_counts, int n_frames, int V, int S, int C);
int mmw_ground_zoom_candidates(mmw_ctx *ctx, const void *d_cubes, const double *d_cand, const int32_t *d_counts,
                               double *d_spec, double *d_zcand, int32_t *d_zcounts, int n_frames, int V, int S, int C,
                               double half_width_m, double hi_cap_m, double fs, double range_max_m);
int mmw_cfar1d_gated(mmw_ctx *ctx, const double *d_mag64, const int32_t *d_gate, uint8_t *d_mask, int32_t *d_dets,
                     int32_t *d_counts, int n_frames, int R, int D, int kind, int num_train, int num_guard, double scale,
                     int k_rank, int cap);
int mmw_cfar1d_rows(mmw_ctx *ctx, const double *d_mag64, const int32_t *d_rows, const int32_t *d_nrows, uint8_t *d_mask,
                    int32_t *d_dets, int32_t *d_counts, int n_frames, int R, int D, int kind, int num_train, int num_guard,
                    double scale, int k_rank, int cap);
int mmw_diag_ground_pick(mmw_ctx *ctx, const double *d_profile, const double *d_bins, double *d_cand, int32_t *d_counts,
                         int n_rows, int S, int max_peaks);

/* Batched RangeDopplerDetectorSequential (range_doppler_detection/range_doppler_detector_sequential.py:72-107 per frame;
 * the detector has no state across frames).  All CFAR arguments are those of mmw_cfar1d, decisions bit-identical to it.
 * mmw_seq_rows: the range CFAR (rng_detector.detect(range_resp), :84-88) on d_profile[F][S] float64, the chirp-0 range
 *   profiles of mmw_range_profile_f64: d_rows[F][S] int32 holds, per frame, the selected range rows in ascending order in
 *   its first d_nrows[f] entries.  One launch, no host round trip.  S <= 3072.
 * mmw_seq_detect: for every frame and every selected row r the float64 Doppler row of virtual antenna 0,
 *   |fftshift_C FFT_C(hann(C)[c] X[r, c])| with X[r, c] = sum_s hann(S)[s] x[0, s, c] exp(-2 pi i r s / S) (the values of
 *   mmw_range_doppler_mag64: range_doppler_resp.py:98-103 and range_doppler_detector.py:78, up to the rounding of a direct
 *   sum against an FFT), the velocity CFAR on it (vel_detector.detect per row, :95-101) and the hits in the order of the
 *   reference's nested comprehension (rows ascending, Doppler ascending == np.where) in d_dets[F][cap][2] / d_counts[F];
 *   counts are exact when a frame overflows cap.  d_cubes is the [F][V][S][C] complex64 batch.  Neither a float64 plane
 *   nor a mask is written.  d_rowmag is NULL, or (to measure the rows against an oracle) [F][S][C] float64 space in which
 *   entry [f][j] receives the Doppler row of range bin d_rows[f][j].  MMW_ERR_UNSUPPORTED (nothing launched) when mmw_seq_route(ctx, S, C) != 0 for the shape alone:
 *   the kernel needs 16 (S + C) + 25 * 4 * max(C, 256) bytes of LDS, at most 160 KiB (S <= 3072 with any C <= 512).
 * mmw_seq_detect_plane: the same result by the plain route: mmw_range_doppler_mag64 of antenna 0 into d_mag64[F][S][C], the
 *   kernel of mmw_cfar1d_gated on the listed rows (d_mask[F][S][C] is work space), mmw_compact2d.
 * Row lists of both: d_nrows[f] below 0 counts as 0 and above S as S (d_rows holds S entries per frame); an entry outside
 *   [0, S) names no row: it gives no detections and adds nothing to d_counts[f] (the d_rowmag entry of such a list position
 *   is not defined).  Lists are ascending, as mmw_seq_rows writes them.
 * mmw_seq_route: 0 when FramePipeline(sequential=...) should call mmw_seq_detect, 1 for mmw_seq_detect_plane: the
 *   context option MMW_SEQ_FULL_PLANE (default 1: the full plane measured faster; 0 asks for the row
 *   kernel) or a shape the row kernel does not serve.  ctx may be NULL (environment and default only). */
int mmw_seq_rows(mmw_ctx *ctx, const double *d_profile, int32_t *d_rows, int32_t *d_nrows, int n_frames, int S, int kind,
                 int num_train, int num_guard, double scale, int k_rank);
int mmw_seq_detect(mmw_ctx *ctx, const void *d_cubes, const int32_t *d_rows, const int32_t *d_nrows, int32_t *d_dets,
                   int32_t *d_counts, int n_frames, int V, int S, int C, int kind, int num_train, int num_guard, double scale,
                   int k_rank, int cap, double *d_rowmag);
int mmw_seq_detect_plane(mmw_ctx *ctx, const void *d_cubes, const int32_t *d_rows, const int32_t *d_nrows, double *d_mag64,
                         uint8_t *d_mask, int32_t *d_dets, int32_t *d_counts, int n_frames, int V, int S, int C, int kind,
                         int num_train, int num_guard, double scale, int k_rank, int cap);
int mmw_seq_route(mmw_ctx *ctx, int S, int C);

/* Device point clouds and batched ego velocity (FramePipeline.point_clouds_device / ego_velocities).
 * mmw_point_cloud: d_points[F][cap][4] float64 (x, y, z, v) of the detections d_dets[F][cap][2] / d_counts[F] and their angle
 *   bins d_az_idx / d_el_idx [F][cap] (either may be NULL: angle 0), as point_cloud_generator.py:216-248 forms them:
 *   x = (rng * cos_el) * cos_az, y = (rng * cos_el) * sin_az, z = rng * sin_el, every product one round-to-nearest multiply
 *   of entries of the caller's float64 tables d_range_bins[S], d_vel_bins[C], d_cos[A], d_sin[A] (np.cos / np.sin of the
 *   angle bins, made on the host).  Slots past a frame's count (counts are clamped to cap) are zeroed.
 * mmw_ego_velocity_ransac: per frame, with N = d_counts[f] points, y = -v and H = p[:dim] / |p[:dim]| (dim 2 or 3), what
 *   RANSACRegressor(LinearRegression(fit_intercept=False), min_samples=10, residual_threshold=thr, max_trials=20,
 *   random_state=42).fit(H, y) of scikit-learn 1.7.2 decides, the refit on the best inlier set, its R^2 on them (0 for at most
 *   3 inliers) and the inlier share: d_out[F][dim + 2].  Zeros when N < 10 or no trial is accepted (the fit's ValueError).
 *   Trial t of a frame fits the points d_subsets[d_subset_row[f]][t][0..9] (the caller's draws of sample_without_replacement for
 *   this N); accepting a trial with k inliers caps the trial count at d_trials_tab[d_trials_off[row] + k] (the caller's
 *   min(20, _dynamic_max_trials(k, N, 10, 0.99)), k = 0 .. N).  n_rows / tab_len: extents of the tables, checked per frame.
 *   d_flags[F]: 0, or the reasons (1 residual at thr, 2 tied scores, 4 R^2 at r2_thr or ill-defined, 8 condition beyond 1e6,
 *   16 non-finite point, 32 table row does not serve N) why the frame's decisions are within rounding of scikit-learn's
 *   SVD solve: its d_out row is zero and the caller recomputes it.  d_inlier_mask: NULL, or [F][cap] uint8.
 *   4 * cap + 48 doubles of LDS: MMW_ERR_UNSUPPORTED beyond 160 KiB. */
int mmw_point_cloud(mmw_ctx *ctx, const int32_t *d_dets, const int32_t *d_counts, const int32_t *d_az_idx, const int32_t *d_el_idx,
                    const double *d_range_bins, const double *d_vel_bins, const double *d_cos, const double *d_sin,
                    double *d_points, int n_frames, int cap, int S, int C, int A);
int mmw_ego_velocity_ransac(mmw_ctx *ctx, const double *d_points, const int32_t *d_counts, int n_frames, int cap, int dim,
                            double thr, double r2_thr, const int32_t *d_subsets, const int32_t *d_subset_row, int n_rows,
                            const int32_t *d_trials_tab, int tab_len, const int32_t *d_trials_off, double *d_out,
                            int32_t *d_flags, uint8_t *d_inlier_mask);

/* mmw_vehicle_velocity_ransac: VehicleVelEstimator.estimate_ego_vel (point_cloud_processing/vehicle_vel_estimator.py) for every
 *   frame of d_points[F][cap][4] / d_counts[F] (the buffers of mmw_ego_velocity_ransac), dim 2 or 3 (only_2D or not).  Per frame:
 *   H = p[:dim] / |p[:dim]|, y = v (no sign change); with an initial estimate the points with (v - H . (-init))^2 <
 *   static_vel_thresh are kept, in order; N of them: below num_close_pts the result is empty.  Iteration i of max_iters fits the
 *   points d_draws[N - points_per_fit][i][0 .. points_per_fit) (the caller's first entries of the i-th rng.permutation(N)) by
 *   dim x dim normal equations, adds every other point whose squared residual is below fit_thresh, and with more than
 *   num_close_pts members refits on all of them; the smallest mean squared error wins, the lowest iteration among equals.
 *   d_init: NULL, or [F][dim] with a NaN in the rows that have no estimate.  chain != 0: d_init is NULL or one row [1][dim], and
 *   ONE workgroup walks the frames in order, every frame taking the last estimate found before it (or the seed row) as its
 *   initial estimate.
 *   d_out[F][dim + 2]: the ego velocity (minus the fit), the mean squared error, N.  d_status[F]: 1 an estimate, 0 the empty
 *   result (d_out holds zeros and N).  d_flags[F]: 0, or MMW_VEHICLE_FLAG_* bits: a decision of the frame lies within rounding of
 *   the host class's, its d_out row is zero, its status 0, and the caller recomputes it.  A flagged frame ends a chain: the frames
 *   behind it carry MMW_VEHICLE_FLAG_CHAIN alone, and the caller goes on from them with the recomputed estimate as the seed.
 *   n_tab: rows of d_draws; a frame whose N has no row, or a row with an entry that is no index below N or is repeated, is
 *   flagged.  LDS: 4 cap + 9 max_iters + 192 doubles; MMW_ERR_UNSUPPORTED beyond 160 KiB.  Every argument is judged before the
 *   context is touched; n_frames == 0 launches nothing. */
#define MMW_VEHICLE_FLAG_RESIDUAL 1    /* a squared residual within the band of fit_thresh */
#define MMW_VEHICLE_FLAG_STATIC 2      /* a squared residual of the static filter within the band of static_vel_thresh */
#define MMW_VEHICLE_FLAG_ERROR_TIE 4   /* an error within the bands of the smallest one, from different members */
#define MMW_VEHICLE_FLAG_COND 8        /* a Gram matrix beyond the condition cap 1e6, or not positive definite */
#define MMW_VEHICLE_FLAG_NONFINITE 16  /* a non-finite point, a point at range 0, an infinite initial estimate */
#define MMW_VEHICLE_FLAG_TABLES 32     /* the draw table does not serve N (caller error; nothing computed) */
#define MMW_VEHICLE_FLAG_CHAIN 64      /* not reached: an earlier frame of the chain was flagged */
int mmw_vehicle_velocity_ransac(mmw_ctx *ctx, const double *d_points, const int32_t *d_counts, int n_frames, int cap, int dim,
                                int points_per_fit, int max_iters, double fit_thresh, int num_close_pts, double static_vel_thresh,
                                const double *d_init, const int32_t *d_draws, int n_tab, int chain, double *d_out, int32_t *d_status,
                                int32_t *d_flags);

/* mmw_detect_batch: the detection pipeline of RangeDopplerDetector2D for a batch of frames in one call:
 *   d_rd[F][V][S][C] c64 (mmw_range_doppler) and, for antenna 0, d_mag64[F][S][C] -> 2-D CFAR mask -> ordered
 *   detections d_dets[F][cap][2] / d_counts[F]
 *   (range_doppler_detection/range_doppler_detector.py:45-80 + range_doppler_detector_2d.py:49-65 per frame).
 *   d_l1 (may be NULL): [F][V] float32, the per-plane norms of mmw_plane_l1 for a following
 *   mmw_angle_argmax_exact -- produced inside the range-Doppler kernel where it can, so the cube is not read again. */
int mmw_detect_batch(mmw_ctx *ctx, const void *d_cubes, void *d_rd, double *d_mag64, uint8_t *d_mask,
                     int32_t *d_dets, int32_t *d_counts, float *d_l1, int n_frames, int V, int S, int C, int cfar_kind,
                     int train_r, int train_d, int guard_r, int guard_d, double scale, int k_rank, int cap);

/* Antenna-integrated (non-coherent) detection.  NO UPSTREAM IMPLEMENTATION: the reference's detectors threshold virtual
 * antenna 0 alone; the definition is DESIGN.md 4.29 and is pinned by a NumPy restatement in the tests.
 * mmw_range_doppler_power64: d_pow[F][S][C] float64 = sum over the n_ants antennas of h_ants (host memory, read during the
 *   call), added in the order of the list, of re^2 + im^2 of the float64 plane mmw_range_doppler_mag64 is defined on,
 *   fftshift_C( FFT_S FFT_C( hann(S) hann(C) x[f][v] ) ).  The order of the sum is the order of the list on every shape, so
 *   one list gives the same bits from run to run; another order of the same antennas agrees to rounding only.  256 x 128
 *   planes in batches of 8 frames and more: one persistent kernel, a frame (every listed antenna) per workgroup (the context
 *   option MMW_POW64_FUSED = 0 turns it off); every other shape and batch: mmw_range_doppler_mag64's own pass per listed
 *   antenna, each followed by d_pow (= | +=) |RD|^2.  Profile family "rd_pow64".
 * mmw_detect_batch_integrated: mmw_detect_batch with that plane in the place of antenna 0's |RD|: d_rd and d_l1 as there,
 *   d_pow[F][S][C] where mmw_detect_batch takes d_mag64, the 2-D CFAR (strict >) on d_pow, the ordered compaction.
 *   MMW_ERR_INVALID (nothing launched, outputs untouched): a null ctx or buffer, a bad shape, h_ants NULL, n_ants outside
 *   1 .. min(V, 32), an index outside [0, V), an index listed twice.  n_frames == 0: MMW_OK, nothing written. */
int mmw_range_doppler_power64(mmw_ctx *ctx, const void *d_cubes, double *d_pow, int n_frames, int V, int S, int C,
                              const int *h_ants, int n_ants);
int mmw_detect_batch_integrated(mmw_ctx *ctx, const void *d_cubes, void *d_rd, double *d_pow, uint8_t *d_mask,
                                int32_t *d_dets, int32_t *d_counts, float *d_l1, int n_frames, int V, int S, int C,
                                int cfar_kind, int train_r, int train_d, int guard_r, int guard_d, double scale, int k_rank,
                                int cap, const int *h_ants, int n_ants);

/* mmw_detect_points: BASELINE configs[2] in one call -- range-Doppler of every antenna (float32, d_rd / d_l1 as above),
 *   CFAR on antenna 0, ordered detections and the azimuth / elevation argmax bins of every detection
 *   (range_doppler_detector.py:62-80, detectors/ca_cfar.py:85-155, point_cloud_generator.py:143-214), with the SAME
 *   results as the float64 path of mmw_detect_batch + mmw_angle_argmax_exact: the CFAR decision is screened on the
 *   float32 plane with a worst-case rounding-error band (mmw_detect.h); the few cells inside the band are decided from
 *   float64 DFT sums of the input cube.  One kernel launch per frame batch behind the range-Doppler kernel instead of six.
 *   d_mag32 (may be NULL): [F][S][C] float32 |RD| of antenna 0.  h_az / h_el: antenna lists (n == 0: that estimate
 *   is skipped and its index buffer may be NULL); d_az_idx / d_el_idx [F][cap] int32.
 *   d_counts[f] is the exact detection count (may exceed cap), or -1 for a frame the screening pass cannot decide
 *   (non-finite samples in antenna 0, or more undecided cells than its list holds): run mmw_detect_batch +
 *   mmw_angle_argmax_exact on such a frame.
 *   h_stats (may be NULL; passing it synchronises): [0] frames with undecided cells, [1] undecided cells, [2] frames
 *   returned with count -1, [3] / [4] azimuth / elevation detections re-evaluated in float64.
 *   MMW_ERR_UNSUPPORTED (nothing launched) when mmw_detect_points_supported(...) == 0: CA-CFAR only, S * C float32
 *   magnitudes must fit the LDS, at most 8 antennas per list -- at most 16 with A = 64 angle bins (the reference's
 *   az_el_fft_size): then the angle estimates are launches of their own in the call's tail, one lane per detection, over
 *   the cells the screening kernel copied aside (the "late argmax", the default whenever A = 64).
 *   The call's tail (exact cells, list insertion, float64 refinement) stays on side queues when the call returns: the
 *   range-Doppler launch of a following mmw_detect_points runs beside it; every other entry point of the context
 *   (mmw_sync, the copies, any other kernel) joins it first, so results are complete whenever they can be observed
 *   through this API.  Context option MMW_DETECT_DEFER_TAIL=0: each call joins its own tail. */
int mmw_detect_points_supported(int S, int C, int cfar_kind, int train_r, int train_d, int guard_r, int guard_d,
                                int n_az, int n_el, int A);
int mmw_detect_points(mmw_ctx *ctx, const void *d_cubes, void *d_rd, float *d_l1, float *d_mag32, int32_t *d_dets,
                      int32_t *d_counts, int32_t *d_az_idx, int32_t *d_el_idx, int n_frames, int V, int S, int C,
                      int cfar_kind, int train_r, int train_d, int guard_r, int guard_d, double scale, int k_rank, int cap,
                      const int *h_az, int n_az, int shift_az, const int *h_el, int n_el, int shift_el, int A,
                      int *h_stats);

/* ---------------------------------------------------------------- point cloud
 * mmw_angle_argmax: for each detection (r, v) of frame f gather rd[f][ant[i]][r][v], zero-pad to A,
 *   FFT, optional fftshift, |.|, first-max argmax (a NaN magnitude wins, as in np.argmax) -> d_idx[F][cap] int32.
 *   replaces PointCloudGenerator._compute_angle_estimation (processors/point_cloud_generator.py:143-214).
 *   float32 arithmetic on the float32 cube: where the reference's two best float64 magnitudes are within ~1e-6 of
 *   each other the index may differ -- the exact variant below removes that.
 * mmw_plane_l1: d_l1[F][V] float32 = sum over each plane of hann(S) hann(C) (|re| + |im|): the scale of the rounding-
 *   error bound the exact variant uses (computed once per batch, shared by the azimuth and elevation calls).
 * mmw_angle_argmax_exact: same result contract as the reference's complex128 computation (:186-206).  The float32
 *   pass bounds how far its magnitudes can be from the float64 ones (from d_l1 and the gathered cells: the WORST-CASE
 *   rounding bound of the kernel that produced the cube -- a proof; the context option MMW_ARGMAX_BOUND_DIV=8 restores
 *   round 3's empirical eighth of it); a detection whose winner is not certainly the float64 one --
 *   best and second-best closer than twice
 *   that bound and, for lists of up to 8 antennas, some bin also failing the pairwise form of the test that treats the two
 *   bins' errors as the same cell errors seen through two steering vectors -- is re-evaluated in float64 from the raw cube
 *   d_cubes (its range-Doppler cells as direct float64 2-D DFT sums, then the float64 angle DFT + argmax).
 *   (mmw_detect_points uses the worst-case bound throughout.)
 *   h_n_refined (may be NULL): number of re-evaluated detections; passing it makes the call synchronise.
 * mmw_angle_argmax_cells64: the float64 angle DFT + first-max argmax for rows of n_ant complex128 cells the caller
 *   gathered itself (a caller-supplied complex128 range-Doppler cube, :168-178); d_cells [n_rows][n_ant].
 * mmw_rd_cells64_at: the complex128 range-Doppler cells the float64 re-evaluation of mmw_angle_argmax_exact works on, read
 *   out for tests: d_out[F][cap][n_ant] complex128 = cell (r, fftshifted Doppler index) of antenna h_ant[i] for every listed
 *   detection (slots from min(d_counts[f], cap) on are left as they were) -- the values the reference's
 *   PointCloudGenerator._compute_angle_estimation gathers from its complex128 cube (processors/point_cloud_generator.py:168-178;
 *   the cube: RangeDopplerProcessor.process, processors/range_doppler_resp.py:49-110).  route = MMW_CELLS64_DENSE: the kernel of the dense refinement (one Doppler FFT per
 *   sample row + range sums; 128 chirps and at most 829 samples, MMW_ERR_UNSUPPORTED otherwise); MMW_CELLS64_DIRECT: the
 *   plane slices of the direct refinement, added in the order the refinement adds them (any plane).  Synchronises (d_out is complete at return); a
 *   listed detection outside the plane is MMW_ERR_INVALID. */
#define MMW_CELLS64_DENSE  0
#define MMW_CELLS64_DIRECT 1
/* MMW_CELLS64_DENSE_MIXED: the dense kernel of the other chirp counts, k_cells64_mixed<C> (C = R1 R2: a register DFT of R1
 *   points per lane, R2 lanes per row) -- the chirp counts mmw_diag_cells64_plan reports, and 128 as well so that it can be
 *   compared with MMW_CELLS64_DENSE on one plane; MMW_ERR_UNSUPPORTED where it has no instantiation or the plane's tables
 *   exceed the LDS.  MMW_CELLS64_DENSE keeps meaning the 128-chirp kernel only. */
#define MMW_CELLS64_DENSE_MIXED 2
int mmw_angle_argmax(mmw_ctx *ctx, const void *d_rd, const int32_t *d_dets, const int32_t *d_counts,
                     int32_t *d_idx, int n_frames, int V, int S, int C, int cap,
                     const int *h_ant, int n_ant, int A, int shift);
int mmw_plane_l1(mmw_ctx *ctx, const void *d_cubes, float *d_l1, int n_frames, int V, int S, int C);
int mmw_angle_argmax_exact(mmw_ctx *ctx, const void *d_cubes, const float *d_l1, const void *d_rd,
                           const int32_t *d_dets, const int32_t *d_counts, int32_t *d_idx, int n_frames,
                           int V, int S, int C, int cap, const int *h_ant, int n_ant, int A, int shift,
                           int *h_n_refined);
int mmw_angle_argmax_cells64(mmw_ctx *ctx, const void *d_cells, int32_t *d_idx, int n_rows, int n_ant, int A,
                             int shift);
int mmw_rd_cells64_at(mmw_ctx *ctx, const void *d_cubes, const int32_t *d_dets, const int32_t *d_counts, void *d_out,
                      int n_frames, int V, int S, int C, int cap, const int *h_ant, int n_ant, int route);

/* TDM-MIMO Doppler phase compensation of the angle estimates.  NO UPSTREAM IMPLEMENTATION: the reference's
 * PointCloudGenerator._compute_angle_estimation transforms the cells as they are.
 * h_phase: host [n_ant][C][2] float64, the factor p[i][c] antenna h_ant[i] is multiplied by in fftshifted Doppler column c
 *   (batch.tdm_phase_table: exp(-2 pi j slot (c - C/2) / (n_slots C))), read during the call.
 * mmw_angle_argmax_tdm: mmw_angle_argmax_exact of the cells z_i p[i][c]: zero-pad to A, FFT, optional fftshift, |.|,
 *   first-max argmax (a NaN magnitude wins) -> d_idx[F][cap] int32.  Counts above cap are clamped, frames with a count <= 0
 *   and the slots from the count on are left as they were, as there.  A float32 pass over d_rd with the worst-case bound of
 *   mmw_angle_argmax_exact (no pairwise form, no MMW_ARGMAX_BOUND_DIV) widened by the rounding of the float32 phasor and
 *   product decides what it can; the rest is re-evaluated in float64: complex128 cells of the direct route of
 *   mmw_rd_cells64_at times the table, angle DFT, argmax.  h_n_refined (may be NULL): their number.  The call synchronises.
 *   A table whose rows are all the same bit for bit (antennas of one transmit slot) is a common phase: the call IS
 *   mmw_angle_argmax_exact then.  MMW_ERR_INVALID: what mmw_angle_argmax_exact refuses, a null h_phase, S > 65535.
 *   MMW_ERR_UNSUPPORTED: (A + distinct rows * C) * 8 bytes beyond 48 KiB of LDS.
 * mmw_angle_argmax_cells64_tdm: the float64 stage alone for cells the caller gathered: d_cells [n_rows][n_ant] complex128,
 *   d_cols [n_rows] int32 the Doppler column of each row (clamped to [0, C)), d_idx [n_rows].  Two bins are ordered on
 *   re^2 + im^2, every operation rounded once (the order of |.| short of overflow).  Synchronises.
 * mmw_diag_angle_argmax_tdm_host: the same stage in plain C++ on host arrays, bit for bit the device's indices; no device
 *   is touched (ctx-free). */
int mmw_angle_argmax_tdm(mmw_ctx *ctx, const void *d_cubes, const float *d_l1, const void *d_rd, const int32_t *d_dets,
                         const int32_t *d_counts, int32_t *d_idx, int n_frames, int V, int S, int C, int cap,
                         const int *h_ant, int n_ant, int A, int shift, const double *h_phase, int *h_n_refined);
int mmw_angle_argmax_cells64_tdm(mmw_ctx *ctx, const void *d_cells, const int32_t *d_cols, const double *h_phase,
                                 int32_t *d_idx, int n_rows, int n_ant, int C, int A, int shift);
int mmw_diag_angle_argmax_tdm_host(const void *h_cells, const int32_t *h_cols, const double *h_phase, int32_t *h_idx,
                                   int n_rows, int n_ant, int C, int A, int shift);

/* TDM-MIMO velocity unwrapping: Doppler hypotheses per detection.  NO UPSTREAM IMPLEMENTATION.
 * A target's Doppler bin is known modulo C: its true bin is k + h C (k = c - C/2) for one h in [0, n_slots), and the
 * compensation above needs the factor of that bin.  h_phase: host [H][n_ant][C][2] float64, one table per hypothesis
 *   (batch.tdm_hypothesis_table: exp(-2 pi j sym(slot (k + h C)) / (n_slots C)), the phase reduced as an integer), read during
 *   the call; 1 <= H <= 8.  A hypothesis whose [n_ant][C] block equals an earlier one's bit for bit, or is, like an earlier
 *   one, a phase common to the whole list (all rows equal bit for bit), is a DUPLICATE: it is never evaluated and stands for
 *   the earlier one.
 * mmw_angle_argmax_tdm_hyp: for every live detection, P_h = max over the A bins of re^2 + im^2 of the DFT of z_i p_h[i][c]
 *   for each distinct h in ascending order; h* = the first maximum over h (a NaN wins); the angle index = the first-maximum
 *   bin of h*, fftshifted with shift.  hyp_given == 0: d_hyp[F][cap] int32 <- h* (its original number), d_idx <- the index.
 *   hyp_given != 0: d_hyp is READ: only hypothesis d_hyp[slot] (clamped to [0, H), a duplicate mapped to the one it
 *   duplicates) is evaluated, d_idx <- its index, d_hyp is left alone.  Counts above cap, frames with a count <= 0 and the
 *   slots from the count on: as mmw_angle_argmax_tdm.  A float32 pass (one lane per detection, every distinct hypothesis in
 *   turn) decides what the rule of mmw_angle_argmax_tdm lets it decide ACROSS all (h, bin) pairs; the rest -- NaN / inf
 *   magnitudes, A == 1 and exact ties between hypotheses included -- is re-evaluated in float64 by that entry's route.
 *   h_n_refined (may be NULL): their number.  The call synchronises.  With one distinct hypothesis the call IS
 *   mmw_angle_argmax_tdm on table 0, and (hyp_given == 0) the live slots of d_hyp are set to 0.
 *   MMW_ERR_INVALID: what mmw_angle_argmax_tdm refuses, a null d_hyp, H < 1, H > 8.
 *   MMW_ERR_UNSUPPORTED: (A + distinct float32 phasor rows * C) * 8 bytes beyond 48 KiB of LDS.
 * mmw_angle_argmax_cells64_tdm_hyp: the float64 stage alone for cells the caller gathered (d_cells [n_rows][n_ant]
 *   complex128, d_cols [n_rows] int32, d_idx / d_hyp [n_rows]).  Synchronises.
 * mmw_diag_angle_argmax_tdm_hyp_host: the same stage in plain C++ on host arrays, bit for bit the device's d_idx and d_hyp;
 *   no device is touched (ctx-free).
 * mmw_tdm_unwrap_velocity: for every live slot of d_points [F][cap][4] float64 (mmw_point_cloud), with c the detection's
 *   Doppler column (outside [0, C): 0, as there), k = c - C/2, M = n_slots C, sym(q) = ((q + M/2) mod M) - M/2 (floor mod),
 *   h = d_hyp[slot] clamped to [0, n_slots): k' = sym(k + h C), m = (k' - k) / C; where m != 0, column 3 <- column 3 +
 *   float64(m) * span (one multiply, one add); where m == 0 the slot is not written.  1 <= n_slots <= 8.  Asynchronous. */
int mmw_angle_argmax_tdm_hyp(mmw_ctx *ctx, const void *d_cubes, const float *d_l1, const void *d_rd, const int32_t *d_dets,
                             const int32_t *d_counts, int32_t *d_idx, int32_t *d_hyp, int hyp_given, int n_frames, int V,
                             int S, int C, int cap, const int *h_ant, int n_ant, int A, int shift, const double *h_phase,
                             int H, int *h_n_refined);
int mmw_angle_argmax_cells64_tdm_hyp(mmw_ctx *ctx, const void *d_cells, const int32_t *d_cols, const double *h_phase, int H,
                                     int32_t *d_idx, int32_t *d_hyp, int hyp_given, int n_rows, int n_ant, int C, int A,
                                     int shift);
int mmw_diag_angle_argmax_tdm_hyp_host(const void *h_cells, const int32_t *h_cols, const double *h_phase, int H,
                                       int32_t *h_idx, int32_t *h_hyp, int hyp_given, int n_rows, int n_ant, int C, int A,
                                       int shift);
int mmw_tdm_unwrap_velocity(mmw_ctx *ctx, double *d_points, const int32_t *d_dets, const int32_t *d_counts,
                            const int32_t *d_hyp, int n_frames, int cap, int C, int n_slots, double span);

/* ---------------------------------------------------------------- beamformers
 * mmw_bartlett: delay-and-sum steering-matrix contraction on MFMA for a batch of frames,
 *   Y[f][s][t] = FFT_S( hann(S) * sum_e X[f][s][e] hamming(E)[e] exp(j 2 pi d_t . p_{f,e} / lambda) )
 *   d_X [F][S][E] c64, d_P [F][3][E] float64 (each frame's array geometry), d_dirs [3][T] float64,
 *   d_out [F][S][T] c64.
 *   replaces compute_synthetic_response / compute_response_at_steering_angle
 *   (processors/simple_synthetic_array_beamformer_processor_multiFrame.py:499-585), whose Python loop over steering
 *   angles (:543-585) becomes one complex GEMM per frame.  d_dirs need not be unit vectors; d_t . p / lambda is reduced modulo
 *   one turn in float64 before anything is narrowed to float32.  MMW_ERR_INVALID, with d_out untouched, for a null ctx, d_X,
 *   d_P, d_dirs or d_out, n_frames outside 0..65535, S, E or T < 1, and a lambda_m that is not > 0 (NaN included);
 *   n_frames == 0 returns MMW_OK and writes nothing.  S = 1 gives the bare contraction (np.hanning(1) == [1.]), S = 2 exact
 *   zeros (that window is all zeros).  A frame whose X or P holds a NaN or an Inf gives non-finite values in that frame's
 *   S x T outputs only.
 * mmw_capon: MVDR spectrum on a V-element half-wavelength ULA for a batch of frames; NO upstream implementation
 *   exists -- definition in DESIGN.md; d_X [F][V][R][K] c64 (K snapshots per range bin),
 *   d_out [F][R][T] float32.  h_thetas: T angles in radians, host memory, read during the call.  MMW_ERR_INVALID, with
 *   d_out untouched, for a null pointer, n_frames < 0, V outside 1..16, R, K or T < 1, and a delta that is negative,
 *   NaN or infinite; n_frames == 0 returns MMW_OK and writes nothing.  delta == 0 with K < V is accepted (the sample
 *   covariance is singular there and the result is not a number the definition gives).  A bin that holds a NaN or an
 *   Inf gives non-finite values in that bin's T outputs only. */
int mmw_bartlett(mmw_ctx *ctx, const void *d_X, const double *d_P, const double *d_dirs,
                 void *d_out, int n_frames, int S, int E, int T, double lambda_m);
int mmw_capon(mmw_ctx *ctx, const void *d_X, const double *h_thetas, float *d_out,
              int n_frames, int V, int R, int K, int T, double delta);
/* mmw_range_snapshots: the snapshots mmw_capon takes as d_X, made from resident cubes d_cubes [F][V][S][C] c64:
 *     d_out[f][i][r - r_lo][k] (complex64, [F][n_rx][r_hi - r_lo][C]) =
 *         sum_s w[s] * x[f][h_rx[i]][s][k] * exp(-2 pi j r s / S),   r_lo <= r < r_hi, every chirp k,
 *     w = np.hanning(S) (the table mmw_range_profile uses) when perform_windowing, else 1.
 *   n_rx == 0: all V antennas in order (as mmw_range_angle); an index may occur more than once in h_rx (host memory, read
 *   during the call).  No upstream implementation exists: the range FFT of every chirp, left in place, is the
 *   [V][R = S][K = C] snapshot tensor of the Capon definition in DESIGN.md.  float32 arithmetic, tables made in float64 on the
 *   host; only the rows of the window are written.  A power-of-two S from 16 to 1024 runs register FFTs with one LDS exchange,
 *   every other S up to 1024 a direct partial DFT whose twiddle index is (r s) mod S in integers.
 *   MMW_ERR_INVALID (nothing launched, d_out untouched; the text names what was refused): a null ctx, d_cubes or d_out,
 *   n_frames < 0, V, S or C < 1, n_rx < 0, n_rx > 0 with a null h_rx, a listed index outside [0, V), a window that is not
 *   0 <= r_lo < r_hi <= S.  MMW_ERR_UNSUPPORTED (nothing launched): S > 1024, or more than 2^31 - 1 workgroups in a launch.
 *   n_frames == 0: MMW_OK, nothing written.  Profile family "range_snapshots". */
int mmw_range_snapshots(mmw_ctx *ctx, const void *d_cubes, void *d_out, int n_frames, int V, int S, int C,
                        const int *h_rx, int n_rx, int r_lo, int r_hi, int perform_windowing);
/* mmw_capon_doppler: the Doppler bin of every detection made on a Capon range-azimuth map, through the MVDR weights of its cell.
 *   No upstream implementation exists; the definition is DESIGN.md 4.28.  d_X [F][n][R][K] complex64 are the
 *   snapshots mmw_capon took (widened exactly to float64 here), d_dets[F][cap][2] int32 (row q of the window, angle index t) and
 *   d_counts[F] what mmw_compact2d wrote for the map; h_thetas: the T angles of the map in radians, host memory, read during
 *   the call.  Per detection, with R_q = X_q X_q^H / K + delta tr(X_q X_q^H / K) / n I and a_i = exp(-j pi i sin(theta_t)):
 *       u = R_q^-1 a,  w = u / Re(a^H u),  y[k] = sum_i conj(w_i) X[i][q][k],  z = fftshift(DFT_K(h y)),
 *   h = np.hanning(K) when doppler_window, else ones:  d_dop[F][cap] = the first index of max |z| (np.argmax), d_peak[F][cap] =
 *   |z[dop]|, d_spec (NULL, or [F][cap][K]) = |z|, d_points (NULL, or [F][cap][4]) = (rng cos(theta_t), rng sin(theta_t), 0,
 *   d_vel[dop]) with rng = d_range[q] (the R rows of the window) -- each product one round-to-nearest multiply, cos / sin of
 *   h_thetas made by the host's C library.  d_range and d_vel [K] may be NULL when d_points is.
 *   A row whose R_q is not positive definite (a Cholesky pivot <= 0 or not finite: an all-zero row, a NaN in the row) gives every
 *   detection of it dop -1, peak NaN, a NaN spectrum and velocity NaN; a detection whose q or t is out of range gives the same
 *   and a NaN position.  Counts are clamped to [0, cap]; slots past a frame's count are zeroed in every output.  The list may
 *   hold its detections in any order.  One workgroup per (frame, row); rows without detections end after reading the list.
 *   MMW_ERR_INVALID (nothing launched, outputs untouched; the text names what was refused): a null ctx, d_X, d_dets, d_counts,
 *   h_thetas, d_dop or d_peak, d_points without d_range and d_vel, n_frames < 0, n outside 1..16, K outside 1..512, R, T or
 *   cap < 1, a delta that is negative, NaN or infinite, a theta that is not finite.  MMW_ERR_UNSUPPORTED (nothing launched):
 *   n_frames * R or n_frames * cap beyond 2^31 - 1.  n_frames == 0: MMW_OK, nothing written.  Profile family "capon_doppler".
 * mmw_diag_capon_doppler_host: the same on host pointers (one implementation of the arithmetic, mmw_capon_doppler.h, and the
 *   same order of every sum: the two agree bit for bit); no context, no device, nothing launched. */
int mmw_capon_doppler(mmw_ctx *ctx, const void *d_X, const int32_t *d_dets, const int32_t *d_counts, const double *h_thetas,
                      int32_t *d_dop, double *d_peak, double *d_spec, double *d_points, const double *d_range, const double *d_vel,
                      int n_frames, int n, int R, int K, int T, int cap, double delta, int doppler_window);
int mmw_diag_capon_doppler_host(const void *h_X, const int32_t *h_dets, const int32_t *h_counts, const double *h_thetas,
                                int32_t *h_dop, double *h_peak, double *h_spec, double *h_points, const double *h_range,
                                const double *h_vel, int n_frames, int n, int R, int K, int T, int cap, double delta,
                                int doppler_window);

/* ---------------------------------------------------------------- element-wise helpers */
int mmw_abs_c64(mmw_ctx *ctx, const void *d_in, float *d_out, size_t n);
/* d_out[i] = (double) d_in[i], n floats (a complex64 array of m elements: n = 2 m): lets a caller that owes the reference's
 *   complex128 / float64 dtypes (range_angle_resp_dbs_enhanced.py:196, range_doppler_resp.py:103) widen on the device and
 *   download the result directly instead of converting on a host core. */
int mmw_widen_f32_f64(mmw_ctx *ctx, const float *d_in, double *d_out, size_t n);

/* ---------------------------------------------------------------- diagnostics
 * In-situ HBM ceiling on the same device: mode 0 = 16-B/lane copy, 1 = write only, 2 = read only,
 * grid-stride over `blocks` workgroups of 256 (0 = 8 per CU).  Used by tools/kbench.py to state what
 * a known-good streaming kernel reaches next to the hot-path kernels. */
/* mmw_diag_set_option: a tuning / test switch of THIS context (the names INTEGRATION.md lists; the same names are read
 *   from the environment when the context has no value of its own).  value == INT_MIN removes the context's value. */
int mmw_diag_set_option(mmw_ctx *ctx, const char *name, int value);
int mmw_diag_membw(mmw_ctx *ctx, const void *d_src, void *d_dst, size_t bytes, int mode, int blocks);
/* Matrix-core peak of this device, measured: back-to-back MFMAs on independent accumulators with register operands,
 * two waves per SIMD.  kind 0 = v_mfma_f32_32x32x2_f32 (the Bartlett GEMM's instruction), 1 = v_mfma_f64_16x16x4_f64
 * (the Capon covariance).  The figure the beamformer kernels' TFLOP/s are divided by in tools/kbench.py.
 * kinds 2 / 3: the kind-0 stream with 8 / 16 independent v_fma_f32 after every MFMA (rate still counts the MFMAs only);
 * kinds 4 / 5: the same with ONE wave per SIMD -- how much vector work hides under float32 MFMAs (it does not);
 * kinds 6 / 7: the contrast case, v_mfma_f32_32x32x16_bf16 alone / with 8 v_fma_f32 after every MFMA (tools/pmc_coexec.sh
 * collects SQ_VALU_MFMA_COEXEC_CYCLES for all of them). */
int mmw_diag_mfma_peak(mmw_ctx *ctx, int kind, double *tflops);
/* Which range-Doppler kernel mmw_range_doppler picks for an S x C plane, without touching a device (host logic
 * only): plan[0] = 0 fused 256x128 | 1 LDS-resident power of two | 2 mixed radix | 3 generic two-kernel path |
 * 4 single pass with half / three quarters of the plane carried in registers (planes of 32768 / 65536 cells);
 * for the mixed-radix kernel plan[1..7] = register class, has a run-time-radix level, S1, S2, C1, C2 (S = S1 S2,
 * C = C1 C2), dynamic LDS bytes.  float64 != 0 asks for the float64 CFAR-plane variant: 2 or 3 by the very test
 * mmw_range_doppler_mag64 makes (power-of-two planes under 8192 cells and planes beyond the LDS: 3; MMW_NO_MIXED_RD = 1
 * in the environment: 3 everywhere); the fused 256 x 128 batch kernel of that entry is not reported.  The float32
 * answer does not read the MMW_NO_*_RD switches. */
int mmw_diag_rd_plan(int S, int C, int float64, int plan[8]);
/* Schedule mmw_chain3d(d_rd = NULL) would use for this batch on this context (host logic + environment knobs only):
 * plan[0] = 1 overlapped (range-Doppler || angle on two queues) / 0 serial, plan[1] = frames per kernel launch,
 * plan[2] = ring depth of range-Doppler chunks in flight, plan[3] = CUs of the range-Doppler queue (0 = unmasked),
 * plan[4] = range-Doppler planes transformed per frame (V, or V - 2 when the zero-weight end antennas of the
 * Hann(V) window are skipped), plan[5] = chain calls of this context re-run on the event schedule after a
 * hand-off timeout so far, plan[6] = 1 for the device-synchronised form (ONE range-Doppler
 * launch and ONE angle launch per call, handing frames over through counters in device memory; plan[1] is then the
 * whole batch), plan[7] = frames in its ring of range-Doppler cubes.  bench.py derives its bytes-per-launch from
 * this instead of restating the rule. */
int mmw_diag_chain_plan(mmw_ctx *ctx, int n_frames, int V, int S, int C, int A, int flags, int plan[8]);

/* Host logic without a device (planning only; what tests/cpp/host_sanitize.cpp runs under ASan / UBSan):
 * mmw_diag_chain_plan_nodev = mmw_diag_chain_plan for a device of num_cu CUs (raw != 0: mmw_chain3d_raw);
 * mmw_diag_detect_plan: banding of mmw_detect_points -- plan[0] supported, [1] workgroups per frame (1), [2] plane rows one
 *   band's loads can carry (band + halo rows), [3] band rows, [4] band pitch, [5] LDS bytes, [6] compile-time window, [7] rounding-error budget of the range-Doppler
 *   kernel for this plane in units of 2^-24 of the plane's L1 norm;
 * mmw_diag_czt_runs: the uniform runs (offset, length, zero-filled) a zoom frequency list of M bins is cut into. */
int mmw_diag_chain_plan_nodev(int num_cu, int raw, int n_frames, int V, int S, int C, int A, int flags, int plan[8]);
int mmw_diag_detect_plan(int S, int C, int cfar_kind, int train_r, int train_d, int guard_r, int guard_d, int n_az,
                         int n_el, int A, int plan[8]);
int mmw_diag_czt_runs(const double *h_freq, int M, int n_used, int *h_runs, int cap, int *n_runs);
/* mmw_diag_cells64_plan: which dense float64 cell kernel the refinement of mmw_angle_argmax_exact has for an S x C plane (host
 *   logic only, no device): plan[0] = 0 none (no instantiation for C, or the tables exceed 160 KiB - 512 B of LDS: the direct
 *   sums serve the plane) | 1 k_cells64<128> | 2 k_cells64_mixed<C>; for 1 and 2 plan[1] = R1 (points per lane), [2] = R2 (lanes
 *   per row; R1 R2 = C), [3] = rows per pass, [4] = dynamic LDS bytes, [5] = cells per chunk, [6] = LDS pitch in complex128
 *   elements; plan[7] = 1 when MMW_CELLS64_DENSE_MIXED of mmw_rd_cells64_at serves the plane (also at C == 128).  Whether
 *   mmw_angle_argmax_exact USES kind 2 is the context option MMW_ARGMAX_DENSE_MIXED. */
int mmw_diag_cells64_plan(int S, int C, int plan[8]);

/* ---------------------------------------------------------------- per-kernel timing hook for bench.py
 * Average duration (ms) of the most recent launch group of the named kernel family measured
 * with HIP event pairs on the launching queue (no host sync): "rd", "angle", "cfar", ...
 * mmw_profile_enable(ctx, n): 0 = off, 1 = time every launch group, n > 1 = every n-th per family
 * (an event pair costs a few microseconds of queue time, so bench.py samples). */
int mmw_profile_enable(mmw_ctx *ctx, int on);
int mmw_profile_get(mmw_ctx *ctx, const char *family, float *total_ms, int *launches);
int mmw_profile_reset(mmw_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* MMWGPU_H */
