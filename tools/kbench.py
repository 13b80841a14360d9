#!/usr/bin/env python3
"""Per-kernel micro-benchmark (HIP events on the ctx stream): angle FFT, range-Doppler, float64 CFAR plane,
CA-CFAR + compaction, next to the in-situ copy / write / read ceilings of the same device.

    python tools/kbench.py [--frames 512] [--reps 10] [--shape 12,63,100]
Prints one JSON object; `GB/s` figures use ALGORITHMIC bytes: a kernel's compulsory read + write.
"""
import argparse
import ctypes as ct
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmwave_radar_processing_amd import _lib  # noqa: E402

V, S, C, A = 12, 256, 128, 64


def timeit(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--shape", default="", help="V,S,C of the cube (default: the headline 12,256,128)")
    args = ap.parse_args()
    global V, S, C
    if args.shape:
        V, S, C = (int(x) for x in args.shape.split(","))
    F = args.frames
    ctx = _lib.Context(0)
    L = ctx.lib
    cube_b, out_b = V * S * C * 8, A * S * C * 8
    d_in, d_rd, d_out = ctx.alloc(F * cube_b), ctx.alloc(F * cube_b), ctx.alloc(F * out_b)
    _lib.check(L.mmw_synth_cubes(ctx.handle, d_in.ptr, F, V, S, C, 99, 8, 30.0))
    res = {"frames": F, "shape": [V, S, C]}
    want = set(args.only.split(",")) if args.only else None

    def run(name, fn, bytes_moved):
        if want and name not in want:
            return
        ms = timeit(ctx, fn, args.reps)
        res[name] = {"ms": round(ms, 4), "us_per_frame": round(1e3 * ms / F, 3),
                     "GBs": round(bytes_moved / ms / 1e6, 1)}

    nbytes = F * out_b
    half = (nbytes // 32) * 16
    run("diag_copy", lambda: _lib.check(L.mmw_diag_membw(ctx.handle, d_out.ptr, d_out.ptr + half, half, 0, 0)), 2 * half)
    run("diag_write", lambda: _lib.check(L.mmw_diag_membw(ctx.handle, d_out.ptr, d_out.ptr, nbytes, 1, 0)), nbytes)
    run("diag_write_angle_pattern", lambda: _lib.check(L.mmw_diag_membw(ctx.handle, d_out.ptr, d_out.ptr, nbytes, 6, 0)), nbytes)
    run("diag_read", lambda: _lib.check(L.mmw_diag_membw(ctx.handle, d_out.ptr, d_out.ptr, nbytes, 2, 0)), nbytes)
    run("rd", lambda: _lib.check(L.mmw_range_doppler(ctx.handle, d_in.ptr, d_rd.ptr, None, F, V, S, C)), F * 2 * cube_b)
    run("angle", lambda: _lib.check(L.mmw_angle_fft(ctx.handle, d_rd.ptr, d_out.ptr, F, V, S, C, A, 0)), F * (cube_b + out_b))
    run("angle_mag", lambda: _lib.check(L.mmw_angle_fft(ctx.handle, d_rd.ptr, d_out.ptr, F, V, S, C, A, 1)),
        F * (cube_b + out_b // 2))
    run("chain3d", lambda: _lib.check(L.mmw_chain3d(ctx.handle, d_in.ptr, None, d_out.ptr, F, V, S, C, A, 0)),
        F * (cube_b + out_b))
    # raw-cube ingest (V = 4 rx x V/4 tx): separate de-interleave pass vs the fused loads
    if V % 4 == 0:
        nrx, ntx = 4, V // 4
        run("reformat", lambda: _lib.check(L.mmw_virtual_array_reformat(ctx.handle, d_in.ptr, d_rd.ptr, F, nrx, ntx, S, C)),
            F * 2 * cube_b)
        run("rd_raw", lambda: _lib.check(L.mmw_range_doppler_raw(ctx.handle, d_in.ptr, d_rd.ptr, F, nrx, ntx, S, C)),
            F * 2 * cube_b)
        run("chain3d_raw", lambda: _lib.check(L.mmw_chain3d_raw(ctx.handle, d_in.ptr, None, d_out.ptr, F, nrx, ntx, S, C, A, 0)),
            F * (cube_b + out_b))
        # int16 (I, Q) raw cubes (layout not pinned by the reference): separate conversion pass vs the loads of the first kernel
        d_iq = ctx.alloc(F * cube_b // 2)
        _lib.check(L.mmw_memset(ctx.handle, d_iq.ptr, 1, F * cube_b // 2))
        run("reformat_i16", lambda: _lib.check(L.mmw_virtual_array_reformat_i16(ctx.handle, d_iq.ptr, d_rd.ptr, F, nrx, ntx, S, C)),
            F * (cube_b // 2 + cube_b))
        run("rd_raw_i16", lambda: _lib.check(L.mmw_range_doppler_raw_i16(ctx.handle, d_iq.ptr, d_rd.ptr, F, nrx, ntx, S, C)),
            F * (cube_b // 2 + cube_b))
        run("chain3d_raw_i16", lambda: _lib.check(L.mmw_chain3d_raw_i16(ctx.handle, d_iq.ptr, None, d_out.ptr, F, nrx, ntx, S, C, A, 0)),
            F * (cube_b // 2 + out_b))
        d_iq.free()
    d_mag = ctx.alloc(F * S * C * 8)
    run("rd_mag64", lambda: _lib.check(L.mmw_range_doppler_mag64(ctx.handle, d_in.ptr, d_mag.ptr, F, V, S, C, 0)),
        F * (S * C * 8 + S * C * 8))
    # antenna-integrated power plane over all V antennas (reads the whole cube, writes one float64 plane per frame): the
    # persistent 256 x 128 kernel, and the per-antenna route (V one-antenna passes + d_pow += |RD|^2) on the same batch
    all_v, n_all = _lib.int_array(range(V))
    pow_call = lambda: _lib.check(L.mmw_range_doppler_power64(ctx.handle, d_in.ptr, d_mag.ptr, F, V, S, C, all_v, n_all))
    run("rd_pow64_all_antennas", pow_call, F * (cube_b + S * C * 8))
    ctx.set_option("MMW_POW64_FUSED", 0)
    run("rd_pow64_all_antennas_per_antenna_route", pow_call, F * (cube_b + S * C * 8))
    ctx.set_option("MMW_POW64_FUSED", None)
    d_thr, d_noise, d_mask = ctx.alloc(F * S * C * 8), ctx.alloc(F * S * C * 8), ctx.alloc(F * S * C)
    alpha = 144 * (1e-5 ** (-1.0 / 144) - 1.0)
    run("cfar2d_ca", lambda: _lib.check(L.mmw_cfar2d(ctx.handle, d_mag.ptr, d_thr.ptr, d_noise.ptr, d_mask.ptr, F, S, C,
                                                     0, 4, 4, 2, 2, alpha, 0)), F * S * C * (8 + 8 + 8 + 1))
    run("cfar2d_ca_maskonly", lambda: _lib.check(L.mmw_cfar2d(ctx.handle, d_mag.ptr, None, None, d_mask.ptr, F, S, C,
                                                              0, 4, 4, 2, 2, alpha, 0)), F * S * C * (8 + 1))
    cap = 1024
    d_dets, d_cnt = ctx.alloc(F * cap * 8), ctx.alloc(F * 4)
    run("compact2d", lambda: _lib.check(L.mmw_compact2d(ctx.handle, d_mask.ptr, d_dets.ptr, d_cnt.ptr, F, S, C, cap)),
        F * S * C)
    k_os = max(1, min(int(0.7 * 200), 200))
    run("cfar2d_os_5x5_g3x2", lambda: _lib.check(L.mmw_cfar2d(ctx.handle, d_mag.ptr, None, None, d_mask.ptr, F, S, C,
                                                               1, 5, 5, 3, 2, 2.0, 122)), F * S * C * (8 + 1))
    # the same detector when thresholds and noise estimates are wanted too: exact order-statistic selection (k_cfar2d)
    run("cfar2d_os_5x5_g3x2_with_thresholds", lambda: _lib.check(L.mmw_cfar2d(
        ctx.handle, d_mag.ptr, d_thr.ptr, d_noise.ptr, d_mask.ptr, F, S, C, 1, 5, 5, 3, 2, 2.0, 122)), F * S * C * (8 + 8 + 8 + 1))
    _lib.check(L.mmw_cfar2d(ctx.handle, d_mag.ptr, None, None, d_mask.ptr, F, S, C, 0, 4, 4, 2, 2, alpha, 0))
    _lib.check(L.mmw_compact2d(ctx.handle, d_mask.ptr, d_dets.ptr, d_cnt.ptr, F, S, C, cap))
    d_idx = ctx.alloc(F * cap * 4)
    ants, n_ant = _lib.int_array(range(8))
    run("angle_argmax_az8", lambda: _lib.check(L.mmw_angle_argmax(ctx.handle, d_rd.ptr, d_dets.ptr, d_cnt.ptr, d_idx.ptr,
                                                                   min(F, 65535), V, S, C, cap, ants, n_ant, A, 1)), F * 8 * 80 * 8)

    def detect_all():
        _lib.check(L.mmw_range_doppler(ctx.handle, d_in.ptr, d_rd.ptr, None, F, V, S, C))
        _lib.check(L.mmw_range_doppler_mag64(ctx.handle, d_in.ptr, d_mag.ptr, F, V, S, C, 0))
        _lib.check(L.mmw_cfar2d(ctx.handle, d_mag.ptr, None, None, d_mask.ptr, F, S, C, 0, 4, 4, 2, 2, alpha, 0))
        _lib.check(L.mmw_compact2d(ctx.handle, d_mask.ptr, d_dets.ptr, d_cnt.ptr, F, S, C, cap))
        _lib.check(L.mmw_angle_argmax(ctx.handle, d_rd.ptr, d_dets.ptr, d_cnt.ptr, d_idx.ptr, min(F, 65535), V, S, C, cap,
                                      ants, n_ant, A, 1))
    run("detect_pipeline_config3", detect_all, F * (2 * cube_b + S * C * 4))

    def detect_batch():
        _lib.check(L.mmw_detect_batch(ctx.handle, d_in.ptr, d_rd.ptr, d_mag.ptr, d_mask.ptr, d_dets.ptr, d_cnt.ptr, None,
                                      min(F, 32768), V, S, C, 0, 4, 4, 2, 2, alpha, 0, cap))
        _lib.check(L.mmw_angle_argmax(ctx.handle, d_rd.ptr, d_dets.ptr, d_cnt.ptr, d_idx.ptr, min(F, 65535), V, S, C, cap,
                                      ants, n_ant, A, 1))
    run("detect_batch_config3", detect_batch, F * (2 * cube_b + S * C * 4))
    d_az, d_el, d_l1p, d_m32 = ctx.alloc(F * cap * 4), ctx.alloc(F * cap * 4), ctx.alloc(F * V * 4), ctx.alloc(F * S * C * 4)
    az8, n_az = _lib.int_array(range(min(8, V)))
    el4, n_el = _lib.int_array(range(max(0, V - 4), V))
    if L.mmw_detect_points_supported(S, C, 0, 4, 4, 2, 2, n_az, n_el, 64):
        run("detect_points_config3", lambda: _lib.check(L.mmw_detect_points(
            ctx.handle, d_in.ptr, d_rd.ptr, d_l1p.ptr, d_m32.ptr, d_dets.ptr, d_cnt.ptr, d_az.ptr, d_el.ptr, F, V, S, C, 0, 4, 4, 2, 2,
            alpha, 0, cap, az8, n_az, 1, el4, n_el, 0, A, None)), F * (2 * cube_b + S * C * 4))
    d_l1 = ctx.alloc(F * V * 4)

    def detect_batch_exact():       # the product path of FramePipeline.point_clouds: exact azimuth argmax
        _lib.check(L.mmw_detect_batch(ctx.handle, d_in.ptr, d_rd.ptr, d_mag.ptr, d_mask.ptr, d_dets.ptr, d_cnt.ptr, d_l1.ptr,
                                      min(F, 32768), V, S, C, 0, 4, 4, 2, 2, alpha, 0, cap))
        _lib.check(L.mmw_angle_argmax_exact(ctx.handle, d_in.ptr, d_l1.ptr, d_rd.ptr, d_dets.ptr, d_cnt.ptr, d_idx.ptr,
                                            min(F, 32768), V, S, C, cap, ants, n_ant, A, 1, None))
    run("detect_batch_config3_exact_argmax", detect_batch_exact, F * (2 * cube_b + S * C * 4))
    run("plane_l1", lambda: _lib.check(L.mmw_plane_l1(ctx.handle, d_in.ptr, d_l1.ptr, F, V, S, C)), F * cube_b)
    run("angle_argmax_exact_az8", lambda: _lib.check(L.mmw_angle_argmax_exact(
        ctx.handle, d_in.ptr, d_l1.ptr, d_rd.ptr, d_dets.ptr, d_cnt.ptr, d_idx.ptr, min(F, 32768), V, S, C, cap, ants, n_ant,
        A, 1, None)), F * 76 * n_ant * 8)
    res["mean_detections_per_frame"] = float(d_cnt.download((F,), np.int32).mean())
    # ---- device point clouds of those detections (angle bins of the exact argmax as azimuth, no elevation list)
    Fp = min(F, 32768)
    tabs = [ctx.alloc(n * 8) for n in (S, C, A, A)]
    for t, n in zip(tabs, (S, C, A, A)):
        t.upload(np.linspace(0.0, 1.0, n))
    d_pts = ctx.alloc(Fp * cap * 32)
    run("point_cloud", lambda: _lib.check(L.mmw_point_cloud(ctx.handle, d_dets.ptr, d_cnt.ptr, d_idx.ptr, None, tabs[0].ptr,
                                                            tabs[1].ptr, tabs[2].ptr, tabs[3].ptr, d_pts.ptr, Fp, cap, S, C, A)),
        Fp * cap * (8 + 4 + 32))
    # ---- Doppler-azimuth: coarse (3-D chain + range mean) and precise (zoom transform, 2 x 128 bins) modes
    Fz = min(F, 256)
    d_mag3 = ctx.alloc(Fz * A * S * C * 4)
    d_da = ctx.alloc(Fz * 2 * C * A * 4)

    def dopaz_coarse():
        _lib.check(L.mmw_chain3d(ctx.handle, d_in.ptr, None, d_mag3.ptr, Fz, V, S, C, A, 1))
        _lib.check(L.mmw_mean_over_range(ctx.handle, d_mag3.ptr, d_da.ptr, Fz, A, S, C, 0, S))
    run("dopaz_coarse_two_pass", dopaz_coarse, Fz * (cube_b + out_b // 2))
    run("dopaz_coarse", lambda: _lib.check(L.mmw_doppler_azimuth(ctx.handle, d_in.ptr, d_da.ptr, Fz, V, S, C, A, 0, S, 0)),
        Fz * cube_b)
    for key in ("dopaz_coarse_two_pass", "dopaz_coarse"):
        if key in res:
            res[key]["us_per_frame"] = round(1e3 * res[key]["ms"] / Fz, 3)
    zf = np.concatenate((np.linspace(0.974, 1.0, C, endpoint=False), np.linspace(0.0, 0.026, C, endpoint=False)))
    run("dopaz_zoom_256bins", lambda: _lib.check(L.mmw_doppler_azimuth_zoom(
        ctx.handle, d_in.ptr, d_da.ptr, Fz, V, S, C, A, 0, S, C, zf.ctypes.data_as(ct.POINTER(ct.c_double)), 2 * C, 0)),
        8.0 * Fz * V * S * C * 2 * C)                          # zoom-transform flops -> GFLOP/s
    if "dopaz_zoom_256bins" in res:
        res["dopaz_zoom_256bins"]["us_per_frame"] = round(1e3 * res["dopaz_zoom_256bins"]["ms"] / Fz, 3)
    d_rz = ctx.alloc(Fz * 256 * 4)
    run("range_zoom_256bins", lambda: _lib.check(L.mmw_range_zoom(ctx.handle, d_in.ptr, d_rz.ptr, Fz, V, S, C, 0, 256, 0.01, 0.0005)),
        Fz * V * S * 8)
    if "range_zoom_256bins" in res:
        res["range_zoom_256bins"]["us_per_frame"] = round(1e3 * res["range_zoom_256bins"]["ms"] / Fz, 3)
    # ---- beamformers (BASELINE config 4 shapes): complex GEMM on f32 MFMA, MVDR covariance on f64 MFMA.
    # "GBs" of these entries is GFLOP/s of USEFUL flops (8 per complex multiply-add); "frac_of_mfma_peak" divides by the
    # matrix-core peak measured on this device by mmw_diag_mfma_peak (the guide lists 157.3 TF f32 MFMA, nothing for f64).
    peak = {}
    for kind, name in ((0, "f32"), (1, "f64")):
        v = ct.c_double(0)
        _lib.check(L.mmw_diag_mfma_peak(ctx.handle, kind, ct.byref(v)))
        peak[name] = v.value
    res["mfma_peak_measured_TFLOPs"] = {k: round(v, 1) for k, v in peak.items()}
    probe = {}
    for kind, name in ((2, "8_fma_per_mfma_2_waves_per_simd"), (3, "16_fma_per_mfma_2_waves_per_simd"),
                       (4, "8_fma_per_mfma_1_wave_per_simd"), (5, "16_fma_per_mfma_1_wave_per_simd"),
                       (6, "bf16_mfma_alone_2_waves_per_simd"), (7, "bf16_mfma_8_fma_per_mfma_2_waves_per_simd")):
        v = ct.c_double(0)
        _lib.check(L.mmw_diag_mfma_peak(ctx.handle, kind, ct.byref(v)))
        probe[name] = round(v.value, 1)
    res["mfma_valu_overlap_probe"] = probe
    rng = np.random.default_rng(1)
    lam = 299792458.0 / 77e9
    for Fb, Sb, Eb, Tb in ((1, 256, 256, 64), (16, 256, 256, 64), (16, 256, 256, 900)):
        X = (rng.standard_normal((Fb, Sb, Eb)) + 1j * rng.standard_normal((Fb, Sb, Eb))).astype(np.complex64)
        d_X = ctx.alloc(X.nbytes); d_X.upload(X)
        d_P = ctx.alloc(Fb * 3 * Eb * 8); d_P.upload(rng.uniform(-0.05, 0.05, (Fb, 3, Eb)))
        az = np.linspace(-1.2, 1.2, Tb)
        dirs = np.ascontiguousarray(np.stack([np.cos(az), np.sin(az), np.zeros(Tb)]))
        d_D = ctx.alloc(dirs.nbytes); d_D.upload(dirs)
        d_Y = ctx.alloc(Fb * Sb * Tb * 8)
        key = f"bartlett_F{Fb}_{Sb}x{Eb}x{Tb}"
        ctx.profile_reset(); ctx.profile_enable(1)
        run(key, lambda: _lib.check(L.mmw_bartlett(ctx.handle, d_X.ptr, d_P.ptr, d_D.ptr, d_Y.ptr, Fb, Sb, Eb, Tb, lam)),
            8.0 * Fb * Sb * Eb * Tb)
        ctx.profile_enable(False)
        if key in res:
            ms, n = ctx.profile_get("cgemm")
            res[key]["us_per_frame"] = round(1e3 * res[key]["ms"] / Fb, 3)
            if n:
                tf = 8.0 * Fb * Sb * Eb * Tb / (ms / n * 1e-3) / 1e12
                res[key]["cgemm_ms"] = round(ms / n, 4)
                res[key]["cgemm_TFLOPs"] = round(tf, 2)
                res[key]["cgemm_frac_of_mfma_peak"] = round(tf / peak["f32"], 3)
        for b_ in (d_X, d_P, d_D, d_Y):
            b_.free()
    Vc, Rc, Kc, Tc = 12, 512, 128, 181
    th = np.linspace(-1.3, 1.3, Tc)
    for Fc in (1, 32):
        d_Xc = ctx.alloc(Fc * Vc * Rc * Kc * 8)
        d_Xc.upload((rng.standard_normal((Fc, Vc, Rc, Kc)) + 1j * rng.standard_normal((Fc, Vc, Rc, Kc))).astype(np.complex64))
        d_Pc = ctx.alloc(Fc * Rc * Tc * 4)
        key = f"capon_F{Fc}_12x512x128_T181"
        # useful flops: covariance 8 V^2 K per bin, forward substitution 8 T V (V + 1) / 2 per bin (no upstream oracle)
        flops = Fc * Rc * (8.0 * Vc * Vc * Kc + 8.0 * Tc * Vc * (Vc + 1) / 2)
        run(key, lambda: _lib.check(L.mmw_capon(ctx.handle, d_Xc.ptr, th.ctypes.data_as(ct.POINTER(ct.c_double)), d_Pc.ptr, Fc,
                                                Vc, Rc, Kc, Tc, 1e-3)), flops)
        if key in res:
            res[key]["us_per_frame"] = round(1e3 * res[key]["ms"] / Fc, 3)
            res[key]["TFLOPs_useful"] = round(flops / (res[key]["ms"] * 1e-3) / 1e12, 2)
            res[key]["frac_of_f64_mfma_peak"] = round(res[key]["TFLOPs_useful"] / peak["f64"], 3)       # measured instruction rate
            res[key]["frac_of_f64_datasheet_78_6TF"] = round(res[key]["TFLOPs_useful"] / 78.6, 3)      # the float64 matrix / vector rate
            res[key]["covariance_mfma_flops_issued"] = Fc * Rc * (Kc // 4) * 4 * 2.0 * 16 * 16 * 4
            res[key]["input_GBs"] = round(Fc * Vc * Rc * Kc * 8 / res[key]["ms"] / 1e6, 1)
        d_Xc.free(); d_Pc.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
