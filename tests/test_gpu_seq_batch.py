"""FramePipeline(sequential=RangeDopplerDetectorSequential): the batched sequential detector against the reference fixtures,
the float64 oracle, the per-frame detector, itself in chunks / streamed / from raw input, by both routes (the row kernel
``mmw_seq_detect``, ``MMW_SEQ_FULL_PLANE=0``, and the full-plane cross-check, ``MMW_SEQ_FULL_PLANE=1``), and the distance of
the row kernel's float64 Doppler rows from the oracle's."""
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from mmwave_radar_processing_amd import _lib, synth
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline, _cfar1d_args
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.processors import PointCloudGenerator
from mmwave_radar_processing_amd.processors.range_doppler_detection import RangeDopplerDetectorSequential
from oracle import oracle_np as O
from test_oracle_golden import GOSO_SEQ, NP2_CASES, NP2_SEEDS, YAML_SEQ, _rd_cases, np2_cfg_text

pytestmark = pytest.mark.gpu

PARAMS = {"yaml": YAML_SEQ, "goso": GOSO_SEQ}
ROUTES = (0, 1)                 # MMW_SEQ_FULL_PLANE
AZ, EL = [0, 3, 4, 7], [9, 8, 5, 4]
SHAPE = (12, 256, 128)
LONG_SEEDS = range(7000, 7208)  # no fixture uses these


def make_cm(text=synth.SYNTH_CFG_256x128x12):
    cm = ConfigManager()
    cm.load_cfg_text(text)
    return cm


def det_kwargs(params):
    rk, rp, vk, vp = params
    return dict(rng_cfar_type=rk, rng_cfar_params=rp, vel_cfar_type=vk, vel_cfar_params=vp)


def pipeline(cm, params, max_frames, shape=SHAPE, az=AZ, el=EL, **kw):
    return FramePipeline(cm, max_frames, shape, sequential=RangeDopplerDetectorSequential(cm, **det_kwargs(params)),
                         az_antenna_idxs=az, el_antenna_idxs=el, **kw)


class route:
    """The context option MMW_SEQ_FULL_PLANE (0: the row kernel, 1: the full plane) for the length of a with block."""

    def __init__(self, full_plane):
        self.value = int(full_plane)

    def __enter__(self):
        _lib.default_context().set_option("MMW_SEQ_FULL_PLANE", self.value)

    def __exit__(self, *exc):
        _lib.default_context().set_option("MMW_SEQ_FULL_PLANE", None)


def assert_dets_equal(got, want, what=""):
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        w = np.asarray(w)
        assert g.dtype == np.int64 and g.ndim == 2 and g.shape[1] == 2, (what, f, g.dtype, g.shape)
        np.testing.assert_array_equal(g, w.reshape(-1, 2), err_msg=f"{what} frame {f}")


def batch_detect(cm, params, cubes, full_plane, shape=SHAPE):
    p = pipeline(cm, params, len(cubes), shape)
    p.load(np.stack(cubes))
    with route(full_plane):
        assert _lib.default_context().lib.mmw_seq_route(_lib.default_context().handle, shape[1], shape[2]) == full_plane
        return p.detect()


@pytest.mark.parametrize("full_plane", ROUTES)
def test_reference_fixtures(full_plane):
    g = np.load(os.path.join(GOLDEN, "detectors_rd.npz"))
    cases = _rd_cases()
    cm = make_cm()
    for name, params in PARAMS.items():
        dets = batch_detect(cm, params, [cube for _, _, cube in cases[:4]], full_plane)
        want = [g[f"s{s}_seq_{name}"] for s in range(4)]
        assert_dets_equal(dets, want, name)
        assert [d.shape[0] for d in dets] == ([134, 167, 139, 127] if name == "yaml" else [14, 48, 9, 32])
        for d, w in zip(dets, want):
            assert d.dtype == w.dtype and d.shape == w.shape
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as fh:
        cm_np2 = make_cm("\n".join(json.load(fh)["6843_RadVel_ods_20Hz.cfg"]["lines"]))
    tag, _, cube = cases[4]
    assert tag == "np2"
    for name, params in PARAMS.items():
        dets = batch_detect(cm_np2, params, [cube], full_plane, cube.shape)
        assert_dets_equal(dets, [g[f"np2_seq_{name}"]], f"np2 {name}")
        assert dets[0].shape == g[f"np2_seq_{name}"].reshape(-1, 2).shape
    assert g["np2_seq_goso"].shape[0] == 0 and dets[0].shape == (0, 2)          # the empty frame
    g2 = np.load(os.path.join(GOLDEN, "detectors_np2.npz"))
    for cfg, shape, _, _ in NP2_CASES:
        tag = "x".join(str(x) for x in shape)
        dets = batch_detect(make_cm(np2_cfg_text(cfg)), YAML_SEQ, [synth.synth_cube(seed, shape) for seed in NP2_SEEDS],
                            full_plane, shape)
        assert_dets_equal(dets, [g2[f"{tag}_s{seed}_seq"] for seed in NP2_SEEDS], tag)


_LONG = {}


def long_cubes():
    if "cubes" not in _LONG:
        _LONG["cubes"] = np.stack([synth.synth_cube(s) for s in LONG_SEEDS])
    return _LONG["cubes"]


def long_run(name):
    """(detections, point clouds, az_idx, el_idx) of the long run in one batch by the row kernel."""
    if name not in _LONG:
        p = pipeline(make_cm(), PARAMS[name], len(LONG_SEEDS))
        p.load(long_cubes())
        with route(0):
            dets = p.detect()
            pcs = p.point_clouds()
        assert_dets_equal(p.dets, dets, "point_clouds().dets")
        _LONG[name] = (dets, pcs, p.az_idx, p.el_idx)
    return _LONG[name]


@pytest.mark.parametrize("name", list(PARAMS))
def test_long_run_matches_oracle_frame_loop_and_other_route(name):
    cubes = long_cubes()
    assert cubes.shape[0] >= 200
    dets, pcs, az_idx, el_idx = long_run(name)
    cm = make_cm()
    params = PARAMS[name]
    # the float64 oracle, detections and argmax bins
    for f, cube in enumerate(cubes):
        want = np.asarray(O.rd_detect_sequential(cube, *params)).reshape(-1, 2)
        np.testing.assert_array_equal(dets[f], want, err_msg=f"oracle frame {f}")
        if len(want):
            raw = O.range_doppler(cube)
            a, _ = O.angle_argmax(raw, want[:, 0], want[:, 1], AZ, 64, True)
            e, _ = O.angle_argmax(raw, want[:, 0], want[:, 1], EL, 64, False)
            np.testing.assert_array_equal(az_idx[f], a, err_msg=f"az frame {f}")
            np.testing.assert_array_equal(el_idx[f], e, err_msg=f"el frame {f}")
        else:
            assert az_idx[f].shape == (0,) and el_idx[f].shape == (0,)
    assert sum(d.shape[0] for d in dets) > 100
    # the per-frame detector and PointCloudGenerator
    det = RangeDopplerDetectorSequential(cm, **det_kwargs(params))
    pcg = PointCloudGenerator(cm, az_antenna_idxs=AZ, el_antenna_idxs=EL, detector_type="range_doppler_detector_sequential",
                              detector_params=det_kwargs(params))
    for f, cube in enumerate(cubes):
        np.testing.assert_array_equal(det.process(cube), dets[f], err_msg=f"process frame {f}")
        want_pc = np.asarray(pcg.process(cube)).reshape(-1, 4)
        assert pcs[f].shape == want_pc.shape
        np.testing.assert_allclose(pcs[f], want_pc, rtol=0, atol=1e-9 * cm.range_max_m, err_msg=f"point cloud frame {f}")
    # the full-plane route gives the same lists
    p = pipeline(cm, params, cubes.shape[0])
    p.load(cubes)
    with route(1):
        other = p.detect()
        other_pcs = p.point_clouds()
    assert_dets_equal(other, dets, "full plane")
    for f in range(cubes.shape[0]):
        np.testing.assert_array_equal(other_pcs[f], pcs[f])
        np.testing.assert_array_equal(p.az_idx[f], az_idx[f])
        np.testing.assert_array_equal(p.el_idx[f], el_idx[f])


@pytest.mark.parametrize("full_plane", ROUTES)
def test_chunks_stream_and_single_frames_agree(full_plane):
    cubes = long_cubes()
    dets, pcs, _, _ = long_run("yaml")
    cm = make_cm()
    sizes = [37, 1, 64, 50, 56]
    assert sum(sizes) == cubes.shape[0]
    bounds = np.cumsum([0] + sizes)
    with route(full_plane):
        ps = pipeline(cm, YAML_SEQ, max(sizes))
        out = list(ps.stream([cubes[a:b] for a, b in zip(bounds[:-1], bounds[1:])], work=lambda q: (q.point_clouds(), q.dets)))
        s_pcs = [pc for o in out for pc in o[0]]
        s_dets = [d for o in out for d in o[1]]
        p1 = pipeline(cm, YAML_SEQ, 1)
        one_pcs, one_dets = [], []
        for cube in cubes[:60]:
            p1.load(cube[None])
            one_pcs += p1.point_clouds()
            one_dets += p1.dets
    assert_dets_equal(s_dets, dets, "stream")
    assert_dets_equal(one_dets, dets[:60], "single frames")
    for f in range(cubes.shape[0]):
        np.testing.assert_array_equal(s_pcs[f], pcs[f])
    for f in range(60):
        np.testing.assert_array_equal(one_pcs[f], pcs[f])


@pytest.mark.parametrize("full_plane", ROUTES)
def test_raw_and_int16_input_on_a_non_power_of_two_shape(full_plane):
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as fh:
        entry = json.load(fh)["6843_RadVel_ods_20Hz.cfg"]
    cm = make_cm("\n".join(entry["lines"]))
    e = entry["expect"]
    num_rx, num_tx, S, C = int(e["num_rx"]), int(e["num_tx"]), int(e["num_samples"]), int(e["loops"])
    shape = (num_rx * num_tx, S, C)
    assert (S, C) == (63, 70)
    # integer-valued samples, so the int16 cube holds exactly the complex64 one
    seq = np.stack([synth.synth_cube(7300 + k, shape) for k in range(24)])
    seq = (np.round(seq.real) + 1j * np.round(seq.imag)).astype(np.complex64)
    assert np.abs(seq.real).max() < 32767 and np.abs(seq.imag).max() < 32767
    raw = np.empty((seq.shape[0], num_rx, S, num_tx * C), dtype=np.complex64)
    for t in range(num_tx):
        raw[:, :, :, t::num_tx] = seq[:, t * num_rx:(t + 1) * num_rx]
    iq = np.stack([raw.real, raw.imag], axis=-1).astype(np.int16)
    total = 0
    for name, params in PARAMS.items():
        want = [np.asarray(O.rd_detect_sequential(cube, *params)).reshape(-1, 2) for cube in seq]
        total += sum(len(w) for w in want)
        with route(full_plane):
            p = pipeline(cm, params, seq.shape[0], shape)
            p.load(seq)
            dets = p.detect()
            pcs = p.point_clouds()
            p2 = pipeline(cm, params, seq.shape[0], shape)
            p2.load_raw(raw, num_tx)
            raw_dets = p2.detect()
            raw_pcs = p2.point_clouds()
            p3 = pipeline(cm, params, seq.shape[0], shape)
            p3.load_raw_i16(iq, num_tx)
            i16_dets = p3.detect()
            i16_pcs = p3.point_clouds()
            p4 = pipeline(cm, params, 7, shape)
            st = list(p4.stream([iq[a:a + 7] for a in range(0, seq.shape[0], 7)], num_tx=num_tx,
                                work=lambda q: (q.point_clouds(), q.dets)))
        assert_dets_equal(dets, want, f"oracle {name}")
        assert_dets_equal(raw_dets, dets, "load_raw")
        assert_dets_equal(i16_dets, dets, "load_raw_i16")
        assert_dets_equal([d for o in st for d in o[1]], dets, "int16 stream")
        st_pcs = [pc for o in st for pc in o[0]]
        for f in range(seq.shape[0]):
            np.testing.assert_array_equal(raw_pcs[f], pcs[f])
            np.testing.assert_array_equal(i16_pcs[f], pcs[f])
            np.testing.assert_array_equal(st_pcs[f], pcs[f])
    assert total > 0


@pytest.mark.parametrize("full_plane", ROUTES)
def test_capacity_exceeded_reports_the_exact_count(full_plane):
    g = np.load(os.path.join(GOLDEN, "detectors_rd.npz"))
    cm = make_cm()
    cubes = np.stack([synth.synth_cube(s) for s in range(4)])
    p = pipeline(cm, YAML_SEQ, 4, det_capacity=150)           # frame 1 holds 167
    p.load(cubes)
    with route(full_plane):
        with pytest.raises(_lib.MmwGpuError, match=r"detection capacity 150 exceeded \(max count 167\)"):
            p.detect()
        np.testing.assert_array_equal(p.counts, [134, 167, 139, 127])
        dets = p.d_dets.download((4, 150, 2), np.int32)
    # what fitted is the head of the full list
    np.testing.assert_array_equal(dets[1], g["s1_seq_yaml"][:150])
    np.testing.assert_array_equal(dets[0, :134], g["s0_seq_yaml"])


def _row_errors(cubes, params):
    """max |rows - oracle| / max(oracle plane) over the selected rows of every frame, for the row kernel and for
    mmw_range_doppler_mag64; and the number of selected rows."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    F, V, S, C = cubes.shape
    det = RangeDopplerDetectorSequential(make_cm(), **det_kwargs(params))
    bufs = _lib.BufferSet(ctx)
    d_in = bufs.get("cubes", F * V * S * C * 8)
    d_in.upload(np.ascontiguousarray(cubes, dtype=np.complex64))
    d_prof, d_rows, d_nrows = bufs.get("prof", F * S * 8), bufs.get("rows", F * S * 4), bufs.get("nrows", F * 4)
    d_dets, d_cnt = bufs.get("dets", F * 4096 * 8), bufs.get("cnt", F * 4)
    d_rowmag, d_mag = bufs.get("rowmag", F * S * C * 8), bufs.get("mag", F * S * C * 8)
    _lib.check(L.mmw_range_profile_f64(h, d_in.ptr, d_prof.ptr, F, V, S, C, 0))
    _lib.check(L.mmw_seq_rows(h, d_prof.ptr, d_rows.ptr, d_nrows.ptr, F, S, *_cfar1d_args(det.rng_detector)))
    _lib.check(L.mmw_seq_detect(h, d_in.ptr, d_rows.ptr, d_nrows.ptr, d_dets.ptr, d_cnt.ptr, F, V, S, C,
                                *_cfar1d_args(det.vel_detector), 4096, d_rowmag.ptr))
    _lib.check(L.mmw_range_doppler_mag64(h, d_in.ptr, d_mag.ptr, F, V, S, C, 0))
    rows, nrows = d_rows.download((F, S), np.int32), d_nrows.download((F,), np.int32)
    rowmag, mag = d_rowmag.download((F, S, C), np.float64), d_mag.download((F, S, C), np.float64)
    bufs.free()
    err_new = err_fft = 0.0
    n_rows = 0
    for f in range(F):
        want = np.abs(O.range_doppler(cubes[f])[0])
        sel = rows[f, :nrows[f]]
        np.testing.assert_array_equal(sel, O.cfar_1d(params[0], O.range_profile(cubes[f], 0), params[1]))
        n_rows += len(sel)
        if len(sel) == 0:
            continue
        scale = want.max()
        err_new = max(err_new, np.abs(rowmag[f, :len(sel)] - want[sel]).max() / scale)
        err_fft = max(err_fft, np.abs(mag[f, sel] - want[sel]).max() / scale)
    return err_new, err_fft, n_rows


def test_row_error_against_the_oracle_stays_within_the_direct_sum_factor():
    """The row kernel forms range bins by direct sums of S terms (and the Doppler row by a direct DFT), mmw_range_doppler_mag64
    by FFTs of log2(S) butterfly stages.  On the selected rows of the fixture frames the row kernel's distance from the
    float64 oracle may exceed the FFT kernel's measured distance by at most S / log2(S), the ratio of the worst-case bounds."""
    cubes = np.stack([synth.synth_cube(s) for s in range(4)])
    S = cubes.shape[2]
    factor = S / math.log2(S)
    for name, params in PARAMS.items():
        err_new, err_fft, n_rows = _row_errors(cubes, params)
        print(f"{name}: {n_rows} selected rows, row kernel {err_new:.3e}, mmw_range_doppler_mag64 {err_fft:.3e}, "
              f"ratio {err_new / err_fft:.2f}, allowed {factor:.1f}")
        assert n_rows > 0 and err_fft > 0
        assert err_new <= factor * err_fft, (name, err_new, err_fft)


def _multi_device_check(devices):
    cm = make_cm()
    cubes = long_cubes()[:50]
    dets, pcs, _, _ = long_run("yaml")
    det = RangeDopplerDetectorSequential(cm, **det_kwargs(YAML_SEQ))
    mp = MultiDeviceFramePipeline(cm, cubes.shape[0], SHAPE, devices=devices, sequential=det, az_antenna_idxs=AZ,
                                  el_antenna_idxs=EL)
    try:
        mp.load(cubes)
        assert mp.bounds[0][1] < cubes.shape[0]                  # really split
        assert_dets_equal(mp.detect(), dets[:50], "multi-device")
        for f, pc in enumerate(mp.point_clouds()):
            np.testing.assert_array_equal(pc, pcs[f])
        assert_dets_equal(mp.dets, dets[:50], "multi-device point_clouds().dets")
    finally:
        mp.close()


def test_three_contexts_of_one_device_equal_single_pipeline():
    _multi_device_check([0, 0, 0])


def test_multi_device_equals_single_pipeline():
    if _lib.device_count() < 2:
        pytest.skip("needs two devices")
    _multi_device_check(None)
