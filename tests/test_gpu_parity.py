"""GPU parity tests: HIP path (through the C ABI) vs the CPU oracle and the committed golden fixtures.

Tolerances (BASELINE.json north_star): spectra max|gpu-ref| / max|ref| <= 1e-5 (fp32 GPU vs the float64
reference); CFAR detection indices bit-exact (values AND order); float64 CFAR thresholds bit-exact when the
float64 input is identical.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from mmwave_radar_processing_amd import synth, _lib
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.detectors import (CaCFAR1D, CaCFAR2D, GoCFAR1D, SoCFAR1D, OsCFAR1D, OsCFAR2D,
                                                   get_detector_registry)
from mmwave_radar_processing_amd.processors import (PointCloudGenerator, RangeAngleProcessor,
                                                    RangeAngleProcessorDBSEnhanced, RangeDopplerProcessor,
                                                    RangeProcessor, VirtualArrayReformatter)
from mmwave_radar_processing_amd.processors.range_doppler_detection import (
    RangeDopplerDetector2D, RangeDopplerDetectorSequential, get_range_doppler_detector_registry)
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu
SPEC_TOL = 1e-5
CFAR = {"num_train": (4, 4), "num_guard": (2, 2), "pfa": 1e-5}


def rel_err(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


CROSS_SCHEDULE_TOL = 1e-6      # max |a - b| / max |b| between two schedules of the same chain (float32 ulps)


def cross_schedule_dev(a, b):
    """Largest element-wise deviation between two schedules' outputs, relative to the frame's peak magnitude."""
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def make_cm(text):
    cm = ConfigManager()
    cm.load_cfg_text(text)
    return cm


def sample_cfg_text():
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as f:
        return "\n".join(json.load(f)["6843_RadVel_ods_20Hz.cfg"]["lines"])


SHAPES = [((12, 32, 16), 101), ((12, 64, 32), 5), ((12, 256, 128), 0), ((12, 63, 70), 202),
          ((4, 128, 64), 9), ((8, 512, 8), 10), ((3, 100, 30), 12),
          # every plane shape of the LDS-resident fused kernel (k_rd_lds)
          ((2, 32, 32), 30), ((2, 64, 32), 31), ((2, 128, 32), 32), ((2, 256, 32), 33), ((3, 512, 32), 34),
          ((2, 32, 64), 35), ((2, 64, 64), 36), ((2, 256, 64), 37), ((2, 32, 128), 38), ((2, 64, 128), 39),
          ((5, 128, 128), 40)]


def test_device_is_gfx950():
    assert "gfx950" in _lib.device_info(0)["arch"]


@pytest.mark.parametrize("shape,seed", SHAPES)
def test_range_doppler_matches_oracle(shape, seed):
    V, S, C = shape
    cm = make_cm(synth.synth_cfg_text(num_samples=S, num_loops=C))
    cube = synth.synth_cube(seed, shape)
    ref = O.range_doppler(cube)
    p = RangeDopplerProcessor(cm)
    got = p.process(cube, rx_idx=-1, return_magnitude=False)
    assert got.dtype == np.complex128 and got.shape == shape
    assert rel_err(got, ref) <= SPEC_TOL
    mag = p.process(cube, rx_idx=V - 1, return_magnitude=True)
    assert mag.dtype == np.float64 and mag.shape == (S, C)
    assert rel_err(mag, np.abs(ref[V - 1])) <= SPEC_TOL
    # unknown kwargs are swallowed (plugin host re-passes ctor params)
    assert p.process(cube, rx_idx=0, some_yaml_key=3).shape == (S, C)


def test_range_doppler_golden_small(golden):
    g = golden("small_chain.npz")
    cm = make_cm(synth.synth_cfg_text(num_samples=32, num_loops=16))
    cube = synth.synth_cube(101, (12, 32, 16))
    p = RangeDopplerProcessor(cm)
    assert rel_err(p.process(cube, rx_idx=-1, return_magnitude=False), g["p2_rd"]) <= SPEC_TOL
    assert rel_err(p.process(cube, rx_idx=3, return_magnitude=True), g["p2_rd_mag_rx3"]) <= SPEC_TOL
    np.testing.assert_array_equal(p.range_bins, g["p2_range_bins"])
    np.testing.assert_array_equal(p.vel_bins, g["p2_vel_bins"])


@pytest.mark.parametrize("shape,seed,A", [((12, 32, 16), 101, 64), ((12, 256, 128), 1, 64), ((12, 63, 70), 202, 64),
                                          ((12, 64, 32), 5, 32), ((8, 64, 32), 6, 64), ((5, 16, 8), 7, 20)])
def test_chain3d_matches_oracle(shape, seed, A):
    V, S, C = shape
    cm = make_cm(synth.synth_cfg_text(num_samples=S, num_loops=C))
    cube = synth.synth_cube(seed, shape)
    p = RangeAngleProcessorDBSEnhanced(cm, num_angle_bins_range_angle_response=A)
    got = p.compute_3d_windowed_fft(cube)
    ref = O.fft3d_windowed(cube, A)
    assert got.shape == (A, S, C) and got.dtype == np.complex128
    assert rel_err(got, ref) <= SPEC_TOL


def test_chain3d_and_dbs_golden(golden):
    g = golden("small_chain.npz")
    cm = make_cm(synth.synth_cfg_text(num_samples=32, num_loops=16))
    cube = synth.synth_cube(101, (12, 32, 16))
    p = RangeAngleProcessorDBSEnhanced(cm, num_angle_bins_range_angle_response=64,
                                       num_angle_bins_dbs_enhanced_response=40)
    assert rel_err(p.compute_3d_windowed_fft(cube), g["p2_fft3d"]) <= SPEC_TOL
    np.testing.assert_array_equal(p.angle_bins_dbs_enhanced, g["p2_dbs_angle_bins"])
    out = p.process(cube, velocity_ned=g["p2_dbs_vel"])
    assert out.shape == g["p2_dbs"].shape and rel_err(out, g["p2_dbs"]) <= SPEC_TOL
    slow = p.process(cube, velocity_ned=np.zeros(3), chirp_idx=2)       # below min_vel_dbs -> plain range-angle
    assert rel_err(slow, g["p2_ra_all"]) <= SPEC_TOL


def test_headline_frames_golden(golden):
    """(12,256,128): detections bit-exact, point cloud, RD / 3-D spectra samples vs the reference's outputs."""
    g = golden("frames_256.npz")
    cm = make_cm(synth.SYNTH_CFG_256x128x12)
    pcg = PointCloudGenerator(cm, az_antenna_idxs=list(range(8)), el_antenna_idxs=[8, 9, 10, 11],
                              detector_type="range_doppler_detector_2d",
                              detector_params={"cfar_type": "ca_cfar_2d", "cfar_params": CFAR}, num_angle_bins=64)
    dbs = RangeAngleProcessorDBSEnhanced(cm)
    np.testing.assert_array_equal(pcg.angle_bins, g["angle_bins"])
    for s in g["seeds"]:
        cube = synth.synth_cube(int(s))
        pc = pcg.process(cube)
        det = pcg.detector
        np.testing.assert_array_equal(det.dets, g[f"s{s}_dets"])
        assert det.dets.dtype == np.int64
        assert rel_err(det.rng_dop_resp_raw[:, ::8, ::8], g[f"s{s}_rd_sample"]) <= SPEC_TOL
        np.testing.assert_allclose(det.detector.thresholds[::4, ::4], g[f"s{s}_thr_sample"], rtol=1e-12)
        np.testing.assert_allclose(det.detector.noise_estimates[::4, ::4], g[f"s{s}_noise_sample"], rtol=1e-12, atol=1e-300)
        if s < 2:
            np.testing.assert_allclose(det.rng_dop_resp, g[f"s{s}_mag0"], rtol=0, atol=1e-12 * np.max(g[f"s{s}_mag0"]))
        assert pc.shape == g[f"s{s}_pc"].shape
        np.testing.assert_allclose(pc, g[f"s{s}_pc"], atol=1e-5 * cm.range_max_m)
        f3 = dbs.compute_3d_windowed_fft(cube)
        m = np.abs(g[f"s{s}_fft3d_checksum"][2])
        assert np.max(np.abs(f3[::4, ::8, ::8] - g[f"s{s}_fft3d_sample"])) / m <= SPEC_TOL
    det2 = RangeDopplerDetector2D(cm, cfar_type="ca_cfar_2d", cfar_params=CFAR)
    d = det2.process(synth.synth_cube(77, num_targets=0))
    assert d.shape == (0, 2) and d.dtype == np.int64


@pytest.mark.parametrize("seed", [20, 21, 22, 23, 24, 25])
def test_detector_and_point_cloud_vs_oracle(seed):
    cm = make_cm(synth.SYNTH_CFG_256x128x12)
    sc = O.cfg_scalars(synth.SYNTH_CFG_256x128x12)
    cube = synth.synth_cube(seed)
    az, el = list(range(8)), [8, 9, 10, 11]
    pcg = PointCloudGenerator(cm, az_antenna_idxs=az, el_antenna_idxs=el,
                              detector_params={"cfar_type": "ca_cfar_2d", "cfar_params": CFAR})
    pc = pcg.process(cube)
    pc_ref, dets_ref, az_i, el_i = O.point_cloud(cube, sc, az, el)
    np.testing.assert_array_equal(pcg.detector.dets, dets_ref)
    raw = O.range_doppler(cube)
    got_az, got_el = pcg._compute_angle_estimation(pcg.detector.rng_dop_resp_raw, dets_ref[:, 0], dets_ref[:, 1])
    # argmax indices identical to the float64 oracle's: the float32 pass re-evaluates every detection it cannot decide
    # within its error bound in float64 from the raw cube (mmw_angle_argmax_exact)
    for got, ref_i in ((got_az, az_i), (got_el, el_i)):
        gi = np.array([int(np.where(pcg.angle_bins == a)[0][0]) for a in got])
        np.testing.assert_array_equal(gi, ref_i)
    # a caller-supplied complex128 cube takes the float64 cell path (mmw_angle_argmax_cells64): same indices again
    got_az2, got_el2 = pcg._compute_angle_estimation(raw, dets_ref[:, 0], dets_ref[:, 1])
    np.testing.assert_array_equal(got_az2, got_az)
    np.testing.assert_array_equal(got_el2, got_el)
    np.testing.assert_allclose(pc, pc_ref, rtol=0, atol=1e-9 * sc["range_max_m"])


def test_exact_argmax_refinement_paths(monkeypatch):
    """mmw_angle_argmax_exact: with the worst-case bound (divisor 1) and with every detection forced through the float64
    path (a huge bound), through the split-plane kernels and through the whole-plane overflow kernel, the indices are the
    oracle's; a NaN cell yields the first NaN bin like np.argmax."""
    from mmwave_radar_processing_amd.batch import FramePipeline
    cm = make_cm(synth.SYNTH_CFG_256x128x12)
    sc = O.cfg_scalars(synth.SYNTH_CFG_256x128x12)
    az, el = list(range(8)), [8, 9, 10, 11]
    cubes = np.stack([synth.synth_cube(8800 + f) for f in range(3)])
    refs = [O.point_cloud(c, sc, az, el) for c in cubes]
    pipe = FramePipeline(cm, max_frames=3, shape=(12, 256, 128), az_antenna_idxs=az, el_antenna_idxs=el)
    pipe.load(cubes)
    n_dets = sum(r[1].shape[0] for r in refs)
    for div, split in (("1", None), ("8", None), ("1", "0"), ("1", "3")):
        monkeypatch.setenv("MMW_ARGMAX_BOUND_DIV", div)
        if split is None:
            monkeypatch.delenv("MMW_REFINE_SPLIT", raising=False)
        else:
            monkeypatch.setenv("MMW_REFINE_SPLIT", split)
        pipe.point_clouds()
        for f, (_, dets_ref, az_i, el_i) in enumerate(refs):
            np.testing.assert_array_equal(pipe.dets[f], dets_ref)
            np.testing.assert_array_equal(pipe.az_idx[f], az_i)
            np.testing.assert_array_equal(pipe.el_idx[f], el_i)
        print(f"bound divisor {div}, split {split}: {pipe.n_refined} of {2 * n_dets} evaluations refined")
        assert 0 <= pipe.n_refined < n_dets
    monkeypatch.delenv("MMW_REFINE_SPLIT", raising=False)
    monkeypatch.delenv("MMW_ARGMAX_BOUND_DIV", raising=False)
    # every detection through the float64 path: the strong component of tests/refine_cases.py in antennas 1 .. 11 raises the
    # bound (the plane norms) while the detector, which reads antenna 0 alone, lists noise-level cells (OS-CFAR: the
    # stand-alone mmw_angle_argmax_exact); split-plane kernels, whole-plane kernels and both in one call
    import refine_cases as rc
    flagged = rc.make_cube(9100, 2, 12, 256, 128)
    flagged[:, 0] = rc.make_cube(9101, 2, 1, 256, 128, 0.0)[:, 0]
    pipe = FramePipeline(cm, max_frames=2, shape=(12, 256, 128), cfar=OsCFAR2D((5, 5), (3, 2), rho=0.7, alpha=2.0),
                         az_antenna_idxs=az, el_antenna_idxs=el)
    pipe.load(flagged)
    assert not pipe._fused_supported(True)
    dets_ref = [O.rd_detect_2d_os(c) for c in flagged]
    n_dets = sum(len(d) for d in dets_ref)
    allowed = rc.allowed_cells(256, 128)
    assert n_dets > 500 and all(np.all(allowed[d[:, 0], d[:, 1]]) for d in dets_ref), "a detection on the strong component"
    for split in (None, "0", "3"):
        if split is None:
            monkeypatch.delenv("MMW_REFINE_SPLIT", raising=False)
        else:
            monkeypatch.setenv("MMW_REFINE_SPLIT", split)
        pipe.point_clouds()
        assert pipe.n_refined == 2 * n_dets, f"{pipe.n_refined} of {2 * n_dets} evaluations refined with P_TONE = {rc.P_TONE:g}"
        for f, d in enumerate(dets_ref):
            np.testing.assert_array_equal(pipe.dets[f], d)
            raw = O.range_doppler(flagged[f])
            for got, ants, shift in ((pipe.az_idx[f], az, True), (pipe.el_idx[f], el, False)):
                want, resp = O.angle_argmax(raw, d[:, 0], d[:, 1], ants, 64, shift)
                top = np.sort(resp, axis=1)[:, -2:]
                sure = top[:, 1] - top[:, 0] >= rc.MARGIN_MIN * top[:, 1]
                assert np.count_nonzero(~sure) <= 0.01 * len(d)
                np.testing.assert_array_equal(got[sure], want[sure])
    monkeypatch.delenv("MMW_REFINE_SPLIT", raising=False)
    # float64 cell path: NaN wins and the first one is reported; +inf beats finite values
    ctx = _lib.default_context()
    cells = np.zeros((3, 4), dtype=np.complex128)
    cells[0] = [1, 2, 3, 4]
    cells[1] = [1, np.nan, 3, 4]
    cells[2] = [np.inf, 0, 0, 0]
    d_cells, d_idx = ctx.alloc(cells.nbytes), ctx.alloc(12)
    d_cells.upload(cells)
    for shift in (0, 1):
        _lib.check(ctx.lib.mmw_angle_argmax_cells64(ctx.handle, d_cells.ptr, d_idx.ptr, 3, 4, 16, shift))
        got = d_idx.download((3,), np.int32)
        spec = np.abs(np.fft.fft(np.pad(cells, ((0, 0), (0, 12))), axis=1))
        if shift:
            spec = np.fft.fftshift(spec, axes=1)
        np.testing.assert_array_equal(got, np.argmax(spec, axis=1))
    d_cells.free()
    d_idx.free()


def test_sample_cfg_non_pow2_pipeline(golden):
    """BASELINE config 1 substitute: the shipped 6843 ODS 20 Hz cfg (12,63,70) end to end on the GPU."""
    g = golden("small_chain.npz")
    cm = make_cm(sample_cfg_text())
    raw = synth.synth_raw_cube(202, 4, 3, 63, 70)
    virt = VirtualArrayReformatter(cm).process(raw)
    assert virt.dtype == np.complex128 and virt.shape == (12, 63, 70)
    np.testing.assert_array_equal(virt[:, ::7, ::9], g["np2_virt_sample"])
    det = RangeDopplerDetector2D(cm, cfar_type="ca_cfar_2d", cfar_params=CFAR)
    dets = det.process(virt)
    np.testing.assert_array_equal(dets, g["np2_dets"])
    assert rel_err(det.rng_dop_resp_raw[:, ::3, ::5], g["np2_rd_sample"]) <= SPEC_TOL
    np.testing.assert_allclose(det.rng_dop_resp, g["np2_mag0"], rtol=0, atol=1e-12 * np.max(g["np2_mag0"]))
    assert det.rng_dop_resp_raw.shape == (12, 63, 70) and det.rng_dop_resp.shape == (63, 70)
    f3 = RangeAngleProcessorDBSEnhanced(cm).compute_3d_windowed_fft(virt)
    m = np.abs(g["np2_fft3d_checksum"][2])
    assert np.max(np.abs(f3[::4, ::3, ::5] - g["np2_fft3d_sample"])) / m <= SPEC_TOL
    raw3 = synth.synth_raw_cube(303, 4, 3, 16, 8)
    cm3 = make_cm(synth.synth_cfg_text(num_samples=16, num_loops=8))
    np.testing.assert_array_equal(VirtualArrayReformatter(cm3).process(raw3), g["var_small"])


def test_range_profile_and_range_angle(golden):
    g = golden("small_chain.npz")
    cm = make_cm(synth.synth_cfg_text(num_samples=32, num_loops=16))
    cube = synth.synth_cube(101, (12, 32, 16))
    assert rel_err(RangeProcessor(cm).process(cube, chirp_idx=5), g["p2_range_profile_c5"]) <= SPEC_TOL
    rap = RangeAngleProcessor(cm, num_angle_bins=64)
    np.testing.assert_array_equal(rap.range_bins, g["p2_ra_range_bins"])
    np.testing.assert_array_equal(rap.angle_bins, g["p2_angle_bins"])
    assert rel_err(rap.process(cube, chirp_idx=2), g["p2_ra_all"]) <= SPEC_TOL
    assert rel_err(rap.process(cube, chirp_idx=0, rx_antennas=[0, 3, 4, 7]), g["p2_ra_sub"]) <= SPEC_TOL
    assert rel_err(rap.process(cube, chirp_idx=1, rx_antennas=np.array([1, 2]), perform_windowing=False),
                   g["p2_ra_nowin"]) <= SPEC_TOL
    # headline and odd shapes against the oracle
    for shape, seed in (((12, 256, 128), 3), ((12, 63, 70), 4)):
        cmx = make_cm(synth.synth_cfg_text(num_samples=shape[1], num_loops=shape[2]))
        c = synth.synth_cube(seed, shape)
        assert rel_err(RangeProcessor(cmx).process(c, chirp_idx=7), O.range_profile(c, 7)) <= SPEC_TOL
        assert rel_err(RangeAngleProcessor(cmx).process(c, chirp_idx=3, rx_antennas=[0, 3, 4, 7]),
                       O.range_angle(c, 64, 3, [0, 3, 4, 7])) <= SPEC_TOL


def test_cfar_known_answers_bit_exact(golden):
    """Reference's verify_detectors_manual.py facts; thresholds bit-exact because the float64 input is identical."""
    g = golden("cfar_known.npz")
    np.random.seed(42)
    x = np.random.exponential(scale=1.0, size=100)
    x[50] = 10.0
    dets = {"ca": CaCFAR1D(10, 2, 1e-3), "go": GoCFAR1D(10, 2, 1e-3), "so": SoCFAR1D(10, 2, 1e-3),
            "os": OsCFAR1D(10, 2, rho=0.75, alpha=5.0), "os_ascalled": OsCFAR1D(10, 2, 15, 5.0)}
    for name, d in dets.items():
        out = d.detect(x)
        assert isinstance(out, list)
        np.testing.assert_array_equal(np.array(out, dtype=np.int64), g[f"1d_{name}_dets"])
        np.testing.assert_array_equal(d.thresholds, g[f"1d_{name}_thr"])
        np.testing.assert_array_equal(d.noise_estimates, g[f"1d_{name}_noise"])
        assert d.detections.dtype == bool
    assert dets["ca"].detect(x) == [50] and dets["os_ascalled"].k_rank == 20
    X = np.random.exponential(scale=1.0, size=(50, 50))
    X[25, 25] = 15.0
    d2 = {"ca": CaCFAR2D((5, 5), (2, 2), 1e-4), "os": OsCFAR2D((5, 5), (2, 2), rho=0.8, alpha=5.0),
          "os_yaml": OsCFAR2D([5, 5], [3, 2], rho=0.7, alpha=2)}
    for name, d in d2.items():
        out = d.detect(X)
        np.testing.assert_array_equal(np.array(out, dtype=np.int64).reshape(-1, 2), g[f"2d_{name}_dets"])
        np.testing.assert_array_equal(d.thresholds, g[f"2d_{name}_thr"])
        np.testing.assert_array_equal(d.noise_estimates, g[f"2d_{name}_noise"])
    assert d2["ca"].detect(X) == [(25, 25)] and d2["os"].k_rank == 160
    assert CaCFAR2D((4, 4), (2, 2), 1e-5).detect(np.ones((5, 5))) == []          # window larger than map
    assert CaCFAR1D(10, 2, 1e-3).detect(np.ones(7)) == []
    assert CaCFAR1D.compute_alpha_ca(20, 1e-3) == 8.250750892455088
    with pytest.raises(ValueError):
        CaCFAR1D(1, 1, 1e-3).detect(np.ones((3, 3)))
    with pytest.raises(ValueError):
        CaCFAR2D((1, 1), (1, 1), 1e-3).detect(np.ones(9))
    assert sorted(get_detector_registry()) == ["ca_cfar_1d", "ca_cfar_2d", "go_cfar_1d", "os_cfar_1d",
                                               "os_cfar_2d", "so_cfar_1d"]


@pytest.mark.parametrize("params", [((4, 4), (2, 2)), ((5, 5), (3, 2)), ((8, 4), (2, 1)), ((1, 1), (0, 0)),
                                    ((2, 9), (1, 3)), ((8, 8), (2, 2)), ((0, 3), (0, 1))])   # (8,8): tile > 1024 cells
def test_cfar2d_random_maps_bit_exact(params):
    rng = np.random.default_rng(hash(params) % 1000)
    X = rng.exponential(1.0, (70, 45)) * 1e3
    X[rng.integers(0, 70, 12), rng.integers(0, 45, 12)] *= 40
    tr, gd = params
    for det, ref in ((CaCFAR2D(tr, gd, 1e-3), O.ca_cfar_2d(X, tr, gd, 1e-3)),
                     (OsCFAR2D(tr, gd, rho=0.7, alpha=3.0), O.os_cfar_2d(X, tr, gd, 0.7, 3.0))):
        out = det.detect(X)
        assert [tuple(map(int, t)) for t in out] == ref[2]
        np.testing.assert_array_equal(det.thresholds, ref[0])
        np.testing.assert_array_equal(det.noise_estimates, ref[1])


@pytest.mark.parametrize("t,g", [(10, 2), (5, 3), (16, 4), (3, 1), (70, 2), (140, 3)])
def test_cfar1d_random_bit_exact(t, g):
    rng = np.random.default_rng(t * 10 + g)
    x = rng.exponential(1.0, 600)
    x[rng.integers(0, 600, 9)] *= 30
    cases = ((CaCFAR1D(t, g, 1e-3), O.ca_cfar_1d(x, t, g, 1e-3)), (GoCFAR1D(t, g, 1e-3), O.go_cfar_1d(x, t, g, 1e-3)),
             (SoCFAR1D(t, g, 1e-3), O.so_cfar_1d(x, t, g, 1e-3)),
             (OsCFAR1D(t, g, rho=0.6, alpha=2.5), O.os_cfar_1d(x, t, g, 0.6, 2.5)))
    for det, ref in cases:
        assert det.detect(x) == ref[2]
        np.testing.assert_array_equal(det.thresholds, ref[0])
        np.testing.assert_array_equal(det.noise_estimates, ref[1])


def test_sequential_detector_vs_oracle():
    cm = make_cm(synth.SYNTH_CFG_256x128x12)
    cube = synth.synth_cube(31)
    rp = dict(num_train=5, num_guard=3, rho=0.6, alpha=2)
    vp = dict(num_train=5, num_guard=2, rho=0.7, alpha=3)
    det = RangeDopplerDetectorSequential(cm, "os_cfar_1d", rp, "os_cfar_1d", vp)
    got = det.process(cube)
    prof = O.range_profile(cube, 0)
    rows = O.os_cfar_1d(prof, 5, 3, 0.6, 2)[2]
    mag = np.abs(O.range_doppler(cube)[0])
    ref = [(r, d) for r in rows for d in O.os_cfar_1d(mag[r], 5, 2, 0.7, 3)[2]]
    ref = np.array(ref, dtype=int) if ref else np.empty((0, 2), dtype=int)
    np.testing.assert_array_equal(got, ref)
    assert got.shape[0] > 0


def test_reference_point_cloud_angle_tests():
    """tests/test_point_cloud_angles.py of the reference, against this package's classes."""
    from unittest.mock import MagicMock
    cm = MagicMock(spec=ConfigManager)
    cm.vel_max_m_s, cm.vel_res_m_s, cm.range_max_m, cm.range_res_m = 10.0, 0.1, 50.0, 0.5
    cm.num_rx_antennas, cm.num_tx_antennas = 4, 3
    params = {"cfar_type": "ca_cfar_2d", "cfar_params": {"num_train": (2, 2), "num_guard": (1, 1), "pfa": 1e-5}}
    raw = np.random.rand(4, 10, 10) + 1j * np.random.rand(4, 10, 10)
    zeros = np.zeros(5, dtype=int)
    for az, el in (([], [0, 1]), ([0, 1], []), ([], [])):
        pc_gen = PointCloudGenerator(config_manager=cm, az_antenna_idxs=az, el_antenna_idxs=el,
                                     detector_type="range_doppler_detector_2d", detector_params=params,
                                     num_angle_bins=64)
        pc_gen.configure()
        a, e = pc_gen._compute_angle_estimation(raw, zeros, zeros)
        assert a.shape == (5,) and e.shape == (5,)
        if not az:
            assert np.all(a == 0.0)
        if not el:
            assert np.all(e == 0.0)
        if el:
            i, _ = O.angle_argmax(raw, zeros, zeros, el, 64, False)
            np.testing.assert_array_equal(e, pc_gen.angle_bins[i])
    with pytest.raises(ValueError):
        PointCloudGenerator(cm, [0], [1], detector_type="nope")
    with pytest.raises(ValueError):
        PointCloudGenerator(cm, "01", [1])
    with pytest.raises(ValueError):
        RangeDopplerDetector2D(cm, cfar_type="nope")
    assert "range_doppler_detector_2d" in get_range_doppler_detector_registry()


def test_compaction_order_and_truncation():
    ctx = _lib.default_context()
    rng = np.random.default_rng(3)
    F, R, D, cap = 3, 37, 29, 50
    mask = (rng.random((F, R, D)) < 0.02).astype(np.uint8)
    mask[1] = 0
    mask[2] = rng.random((R, D)) < 0.2          # overflows cap
    d_m, d_d, d_c = ctx.alloc(mask.nbytes), ctx.alloc(F * cap * 8), ctx.alloc(F * 4)
    d_m.upload(mask)
    _lib.check(ctx.lib.mmw_compact2d(ctx.handle, d_m.ptr, d_d.ptr, d_c.ptr, F, R, D, cap))
    counts = d_c.download((F,), np.int32)
    dets = d_d.download((F, cap, 2), np.int32)
    for f in range(F):
        rows, cols = np.where(mask[f])
        assert counts[f] == len(rows)
        n = min(cap, len(rows))
        np.testing.assert_array_equal(dets[f, :n, 0], rows[:n])
        np.testing.assert_array_equal(dets[f, :n, 1], cols[:n])
    assert counts[1] == 0 and counts[2] > cap
    for b in (d_m, d_d, d_c):
        b.free()


def test_synth_kernel_frames_feed_the_oracle():
    """Bench input path: cubes generated in HBM are integer-valued, and the chain on them matches the oracle."""
    ctx = _lib.default_context()
    F, V, S, C, A = 3, 12, 256, 128, 64
    n = V * S * C
    d_in, d_out = ctx.alloc(F * n * 8), ctx.alloc(F * A * S * C * 8)
    _lib.check(ctx.lib.mmw_synth_cubes(ctx.handle, d_in.ptr, F, V, S, C, 1234, 8, 30.0))
    _lib.check(ctx.lib.mmw_chain3d(ctx.handle, d_in.ptr, None, d_out.ptr, F, V, S, C, A, 0))
    cubes = d_in.download((F, V, S, C), np.complex64)
    assert np.all(cubes.real == np.rint(cubes.real)) and np.all(cubes.imag == np.rint(cubes.imag))
    assert 20 < np.std(cubes.real) < 2000 and not np.array_equal(cubes[0], cubes[1])
    out = d_out.download((F, A, S, C), np.complex64)
    for f in (0, 2):
        assert rel_err(out[f], O.fft3d_windowed(cubes[f], A)) <= SPEC_TOL
    d_in.free()
    d_out.free()


def test_bartlett_mfma_matches_reference_golden(golden):
    from mmwave_radar_processing_amd.processors.steering_beamformers import SyntheticArrayBeamformerCore
    g = golden("bartlett_small.npz")
    rng = np.random.default_rng(404)
    frames, S, chirps = 2, 64, 24
    hist = rng.standard_normal((frames, S, chirps)) + 1j * rng.standard_normal((frames, S, chirps))
    geom = rng.uniform(-0.02, 0.02, (frames, 3, chirps))
    bf = SyntheticArrayBeamformerCore(g["az"], g["el"], float(g["lambda_m"]))
    np.testing.assert_array_equal(bf.d, g["d"])
    out = bf.compute_synthetic_response(hist, geom)
    assert out.shape == g["out"].shape and out.dtype == np.complex128
    assert rel_err(out, g["out"]) <= SPEC_TOL


@pytest.mark.parametrize("S,E,naz,nel", [(256, 256, 60, 1), (128, 100, 33, 3), (70, 37, 5, 2)])
def test_bartlett_mfma_vs_oracle_shapes(S, E, naz, nel):
    from mmwave_radar_processing_amd.processors.steering_beamformers import SyntheticArrayBeamformerCore
    rng = np.random.default_rng(S + E)
    X = (rng.standard_normal((S, E)) + 1j * rng.standard_normal((S, E))).astype(np.complex64)
    P = rng.uniform(-0.05, 0.05, (3, E))
    az, el = np.linspace(-1.2, 1.2, naz), np.linspace(-0.4, 0.4, nel)
    lam = 299792458.0 / 77e9
    bf = SyntheticArrayBeamformerCore(az, el, lam)
    out = bf.contract(X, P)
    ref = O.bartlett_response(X.astype(complex), P, O.steering_dirs(az, el), lam)
    assert rel_err(out, ref) <= SPEC_TOL
    # a batch of frames, each with its own array geometry, in one launch group == frame by frame
    Xb = np.stack([X, X[::-1], 2.0 * X])
    Pb = np.stack([P, rng.uniform(-0.05, 0.05, (3, E)), P])
    outb = bf.contract(Xb, Pb)
    assert outb.shape == (3,) + out.shape
    np.testing.assert_array_equal(outb[0], out)
    assert rel_err(outb[1], O.bartlett_response(Xb[1].astype(complex), Pb[1], O.steering_dirs(az, el), lam)) <= SPEC_TOL
    assert rel_err(outb[2], 2.0 * ref) <= SPEC_TOL


def test_bartlett_both_contraction_paths():
    """The steering-matrix contraction has two kernels: the fused tile kernel (small problems: steering evaluated in the
    kernel) and the LDS-tiled GEMM behind k_steer (large ones).  A problem big enough for the second by default, and the small
    shapes forced through each path, through the polynomial sine / cosine variant of the tile kernel, through its 16 x 16-tile
    form (the default for a frame or two) and through the float32-MFMA form (context options)."""
    from mmwave_radar_processing_amd.processors.steering_beamformers import SyntheticArrayBeamformerCore
    rng = np.random.default_rng(77)
    S, E = 512, 128
    az, el = np.linspace(-1.2, 1.2, 300), np.linspace(-0.4, 0.4, 3)            # 900 directions: 48 x 29 tiles of 32 x 32
    lam = 299792458.0 / 77e9
    X = (rng.standard_normal((3, S, E)) + 1j * rng.standard_normal((3, S, E))).astype(np.complex64)
    P = rng.uniform(-0.05, 0.05, (3, 3, E))
    out = SyntheticArrayBeamformerCore(az, el, lam).contract(X, P)
    for f in range(3):
        assert rel_err(out[f], O.bartlett_response(X[f].astype(complex), P[f], O.steering_dirs(az, el), lam)) <= SPEC_TOL
    ctx = _lib.default_context()
    for knobs in ({"MMW_BARTLETT_PATH": 2}, {"MMW_BARTLETT_PATH": 1, "MMW_BARTLETT_TILE16": 0}, {"MMW_BARTLETT_PATH": 1, "MMW_BARTLETT_POLY": 1},
                  {"MMW_BARTLETT_PATH": 1, "MMW_BARTLETT_TILE16": 1}, {"MMW_BARTLETT_PATH": 1, "MMW_BARTLETT_BF16": 0}):
        for k, v in knobs.items():
            ctx.set_option(k, v)
        try:
            worst = 0.0
            for S2, E2, naz, nel in ((256, 256, 60, 1), (128, 100, 33, 3), (70, 37, 5, 2)):
                rng2 = np.random.default_rng(S2 + E2)
                X2 = (rng2.standard_normal((2, S2, E2)) + 1j * rng2.standard_normal((2, S2, E2))).astype(np.complex64)
                P2 = rng2.uniform(-0.05, 0.05, (2, 3, E2))
                az2, el2 = np.linspace(-1.2, 1.2, naz), np.linspace(-0.4, 0.4, nel)
                out2 = SyntheticArrayBeamformerCore(az2, el2, lam, ctx=ctx).contract(X2, P2)
                for f in range(2):
                    ref = O.bartlett_response(X2[f].astype(complex), P2[f], O.steering_dirs(az2, el2), lam)
                    worst = max(worst, float(np.abs(out2[f] - ref).max() / np.abs(ref).max()))
        finally:
            for k in knobs:
                ctx.set_option(k, None)
        print(f"bartlett {knobs}: worst deviation {worst:.2e} of the peak")
        assert worst <= SPEC_TOL


def test_capon_mfma_vs_own_oracle():
    """BASELINE config 4 shape: 12-element array x 512 range bins.  NO UPSTREAM ORACLE (the reference has no Capon code,
    SURVEY.md F2): parity unpinned -- checked against this build's own float64 definition (oracle_np.capon_spectrum),
    a single-source peak, the batch entry point, odd sizes, and an analytic two-source resolution case."""
    from mmwave_radar_processing_amd.processors.steering_beamformers import CaponBeamformer
    import capon_cases as cc

    def assert_capon_bound(P, X, th, delta):
        """|P - ref| <= (2^-23 + (C_KERNEL + C_ORACLE) cond2 2^-53) |ref|, cond2 per range bin (tests/capon_cases.py)"""
        ref = O.capon_spectrum(X, th, delta=delta)
        tol = cc.bound(cc.cond2(X[None], delta)[0])[:, None]
        assert np.all(np.abs(P - ref) <= tol * np.abs(ref)), float(np.max(np.abs(P - ref) / (tol * np.abs(ref))))

    rng = np.random.default_rng(8)
    V, R, K = 12, 512, 128
    th = np.linspace(-1.3, 1.3, 181)
    th0 = rng.uniform(-1.0, 1.0, R)
    a = np.exp(-1j * np.pi * np.arange(V)[:, None] * np.sin(th0)[None, :])          # [V, R]
    s = rng.standard_normal((R, K)) + 1j * rng.standard_normal((R, K))
    X = (a[:, :, None] * s[None] * 8 + rng.standard_normal((V, R, K)) + 1j * rng.standard_normal((V, R, K)))
    X = X.astype(np.complex64)
    cap = CaponBeamformer(th, delta=1e-3)
    P = cap.process(X)
    assert P.shape == (R, len(th))
    assert_capon_bound(P, X, th, 1e-3)
    assert np.all(np.abs(th[np.argmax(P, axis=1)] - th0) <= 0.03)
    # batch of frames in one launch == frame by frame
    Xb = np.stack([X, X[:, ::-1, :], 0.5 * X])
    Pb = cap.process(Xb)
    assert Pb.shape == (3, R, len(th))
    np.testing.assert_array_equal(Pb[0], P)
    np.testing.assert_array_equal(Pb[1], P[::-1])
    np.testing.assert_allclose(Pb[2], 0.25 * P, rtol=1e-6)       # P scales with the signal power (float32 output)
    # odd sizes: 7 antennas, 5 range bins, 37 snapshots (partial staging tile, odd K), 70 angles
    X2 = (rng.standard_normal((2, 7, 5, 37)) + 1j * rng.standard_normal((2, 7, 5, 37))).astype(np.complex64)
    th2 = np.linspace(-1.0, 1.0, 70)
    P2 = CaponBeamformer(th2, delta=1e-2).process(X2)
    for f in range(2):
        assert_capon_bound(P2[f], X2[f], th2, 1e-2)
    # sixteen antennas (four register rows per lane), 200 angles (beyond the 192 held in the LDS table), K = 96 and K = 33
    for Vn, Kn in ((16, 96), (13, 33), (3, 64), (1, 32)):
        X3 = (rng.standard_normal((2, Vn, 9, Kn)) + 1j * rng.standard_normal((2, Vn, 9, Kn))).astype(np.complex64)
        th3 = np.linspace(-1.2, 1.2, 200)
        P3 = CaponBeamformer(th3, delta=1e-2).process(X3)
        for f in range(2):
            assert_capon_bound(P3[f], X3[f], th3, 1e-2)
    # two uncorrelated sources 0.12 rad apart: closer than the Rayleigh width of a 12-element half-wavelength array
    # (2 / V = 0.17 in sin(theta)), so the delay-and-sum (Bartlett) spectrum shows ONE lobe while the MVDR spectrum,
    # whose peak width shrinks with SNR, shows two peaks at the source angles with a dip between them.  With exact
    # covariance R = sigma_s^2 (a1 a1^H + a2 a2^H) + sigma_n^2 I the MVDR spectrum has the closed form below.
    t1, t2 = -0.06, 0.06
    a1 = np.exp(-1j * np.pi * np.arange(V) * np.sin(t1))
    a2 = np.exp(-1j * np.pi * np.arange(V) * np.sin(t2))
    Kb = 4096
    s1 = (rng.standard_normal(Kb) + 1j * rng.standard_normal(Kb)) * np.sqrt(50.0)
    s2 = (rng.standard_normal(Kb) + 1j * rng.standard_normal(Kb)) * np.sqrt(50.0)
    Xt = a1[:, None] * s1 + a2[:, None] * s2 + (rng.standard_normal((V, Kb)) + 1j * rng.standard_normal((V, Kb))) * np.sqrt(0.5)
    tht = np.linspace(-0.4, 0.4, 321)
    Pt = CaponBeamformer(tht, delta=0.0).process(Xt[:, None, :].astype(np.complex64))[0]
    At = np.exp(-1j * np.pi * np.arange(V)[:, None] * np.sin(tht)[None, :])
    Rth = 100.0 * (np.outer(a1, a1.conj()) + np.outer(a2, a2.conj())) + 1.0 * np.eye(V)
    Pth = 1.0 / np.real(np.sum(At.conj() * np.linalg.solve(Rth, At), axis=0))
    i1, i2, im = np.argmin(np.abs(tht - t1)), np.argmin(np.abs(tht - t2)), np.argmin(np.abs(tht))
    peaks = [i for i in range(1, len(tht) - 1) if Pt[i] > Pt[i - 1] and Pt[i] > Pt[i + 1] and Pt[i] > 0.2 * Pt.max()]
    assert len(peaks) == 2 and abs(peaks[0] - i1) <= 2 and abs(peaks[1] - i2) <= 2          # resolved, at the sources
    assert Pt[im] < 0.5 * min(Pt[i1], Pt[i2])                                                  # a real dip between them
    np.testing.assert_allclose(Pt[[i1, i2, im]], Pth[[i1, i2, im]], rtol=0.15)                 # finite-sample covariance
    bart = np.abs(At.conj().T @ Xt.astype(np.complex64)).mean(axis=1)
    bpk = [i for i in range(1, len(tht) - 1) if bart[i] > bart[i - 1] and bart[i] > bart[i + 1] and bart[i] > 0.5 * bart.max()]
    assert len(bpk) == 1                                                                       # delay-and-sum does not resolve them


def test_frame_pipeline_matches_per_frame_processors_and_oracle():
    """BASELINE configs[2]/[4]: batch of cubes resident in HBM -> detections + point clouds, frame by frame identical
    to the single-frame processors and to the oracle; then the same through the shard split."""
    from mmwave_radar_processing_amd.batch import FramePipeline, run_sharded, shard_bounds
    cm = make_cm(synth.SYNTH_CFG_256x128x12)
    sc = O.cfg_scalars(synth.SYNTH_CFG_256x128x12)
    az, el = list(range(8)), [8, 9, 10, 11]
    F = 6
    cubes = np.stack([synth.synth_cube(40 + f) for f in range(F)])
    pipe = FramePipeline(cm, max_frames=8, shape=(12, 256, 128), cfar=CaCFAR2D((4, 4), (2, 2), 1e-5),
                         az_antenna_idxs=az, el_antenna_idxs=el)
    pipe.load(cubes)
    pcs = pipe.point_clouds()
    pcg = PointCloudGenerator(cm, az_antenna_idxs=az, el_antenna_idxs=el,
                              detector_params={"cfar_type": "ca_cfar_2d", "cfar_params": CFAR})
    for f in range(F):
        pc_ref, dets_ref, _, _ = O.point_cloud(cubes[f], sc, az, el)
        np.testing.assert_array_equal(pipe.dets[f], dets_ref)
        assert pipe.dets[f].dtype == np.int64
        single = pcg.process(cubes[f])
        np.testing.assert_array_equal(pcs[f], single)            # same kernels, same bits
        np.testing.assert_allclose(pcs[f], pc_ref, rtol=0, atol=1e-9 * sc["range_max_m"])
    pipe.chain3d()
    for f in (0, F - 1):
        assert rel_err(pipe.fetch_chain3d(f), O.fft3d_windowed(cubes[f])) <= SPEC_TOL
    # OS-CFAR variant of the detector on the same batch
    pipe_os = FramePipeline(cm, max_frames=8, shape=(12, 256, 128), cfar=OsCFAR2D((5, 5), (3, 2), rho=0.7, alpha=4.0))
    pipe_os.load(cubes[:2])
    d_os = pipe_os.detect()
    for f in range(2):
        mag = np.abs(O.range_doppler(cubes[f])[0])
        ref = O.os_cfar_2d(mag, (5, 5), (3, 2), 0.7, 4.0)[2]
        np.testing.assert_array_equal(d_os[f], np.array(ref, dtype=np.int64).reshape(-1, 2))
    # shard split: two "ranks" processed one after the other give the same frames in order
    parts = []
    for r in range(2):
        lo, hi = shard_bounds(F, r, 2)
        pipe.load(cubes[lo:hi])
        parts.extend(pipe.detect())
    for f in range(F):
        np.testing.assert_array_equal(parts[f], O.rd_detect_2d(cubes[f])[2])
    # synthetic frames generated in HBM, checked through the oracle on the downloaded bytes
    pipe.synth(5, seed0=31337)
    dets = pipe.detect()
    dl = pipe.cubes()
    for f in (0, 4):
        np.testing.assert_array_equal(dets[f], O.rd_detect_2d(dl[f])[2])
    with pytest.raises(_lib.MmwGpuError):
        small = FramePipeline(cm, max_frames=2, shape=(12, 256, 128), det_capacity=4)
        small.load(cubes[:1])
        small.detect()


def test_multi_device_pipeline_matches_single_pipeline():
    """One process, one host thread + context per device.  Runs on however many devices are visible and,
    to exercise the split / join with a single GPU too, on three contexts of device 0."""
    from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline
    cm = make_cm(synth.synth_cfg_text(num_samples=64, num_loops=32))
    shape, F = (12, 64, 32), 11
    cfar = CaCFAR2D((4, 4), (2, 2), 1e-4)
    kw = dict(cfar=cfar, az_antenna_idxs=list(range(8)), el_antenna_idxs=[8, 9, 10, 11], det_capacity=512)
    cubes = np.stack([synth.synth_cube(4000 + f, shape, num_targets=4) for f in range(F)])
    single = FramePipeline(cm, max_frames=F, shape=shape, **kw)
    single.load(cubes)
    pcs_ref = single.point_clouds()
    dets_ref = single.dets
    single.chain3d()
    for devices in (None, [0, 0, 0]):
        mp = MultiDeviceFramePipeline(cm, max_frames=F, shape=shape, devices=devices, **kw)
        assert mp.world == (_lib.device_count() if devices is None else 3)
        mp.load(cubes)
        pcs = mp.point_clouds()
        assert len(pcs) == F
        for f in range(F):
            np.testing.assert_array_equal(mp.dets[f], dets_ref[f])
            np.testing.assert_array_equal(pcs[f], pcs_ref[f])
        out = np.zeros((F, 64) + shape[1:], dtype=np.complex64)
        mp.chain3d(out=out)
        for f in (0, F // 2, F - 1):
            np.testing.assert_array_equal(out[f], single.fetch_chain3d(f))
            np.testing.assert_array_equal(mp.fetch_chain3d(f), out[f])
        # device-generated frames: frame f comes from seed0 + f wherever it lands
        mp.synth(F, seed0=77000)
        single.synth(F, seed0=77000)
        np.testing.assert_array_equal(mp.cubes(), single.cubes())
        a, b = mp.detect(), single.detect()
        for f in range(F):
            np.testing.assert_array_equal(a[f], b[f])
        mp.close()
        single.load(cubes)


def test_overlapped_chain_schedule_full_batch():
    """The default schedule for large batches (RD and angle kernels on CU-masked queues, 40-frame chunks,
    lazy join with the context stream): every chunk boundary, the tail chunk and back-to-back calls are
    checked against the oracle, with unrelated work interleaved on the context stream."""
    ctx = _lib.default_context()
    F, V, S, C, A = 330, 12, 256, 128, 64
    n = V * S * C
    d_in, d_out, d_rd = ctx.alloc(F * n * 8), ctx.alloc(F * A * S * C * 8), ctx.alloc(4 * n * 8)
    L, h = ctx.lib, ctx.handle
    check_frames = (0, 39, 40, 41, 79, 80, 159, 160, 319, 320, 329)

    def verify(cubes):
        for f in check_frames:
            got = d_out.download((A, S, C), np.complex64, f * A * S * C * 8)
            assert rel_err(got, O.fft3d_windowed(cubes[f], A)) <= SPEC_TOL, f

    for rnd, seed in enumerate((555, 777)):
        _lib.check(L.mmw_synth_cubes(h, d_in.ptr, F, V, S, C, seed, 8, 30.0))
        d_out.zero()
        _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_out.ptr, F, V, S, C, A, 0))
        if rnd == 1:    # a second chain right behind the first (pipeline kept full), then other work
            _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_out.ptr, F, V, S, C, A, 0))
            _lib.check(L.mmw_range_doppler(h, d_in.ptr, d_rd.ptr, None, 4, V, S, C))
        cubes = d_in.download((F, V, S, C), np.complex64)
        verify(cubes)
        if rnd == 1:
            rd = d_rd.download((4, V, S, C), np.complex64)
            assert rel_err(rd[3], O.range_doppler(cubes[3])) <= SPEC_TOL
    # magnitude output through the same schedule
    _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_out.ptr, F, V, S, C, A, 1))
    for f in (0, 200, 329):
        got = d_out.download((A, S, C), np.float32, f * A * S * C * 4)
        assert rel_err(got, np.abs(O.fft3d_windowed(cubes[f], A))) <= SPEC_TOL
    for b in (d_in, d_out, d_rd):
        b.free()


def test_degenerate_shapes_and_arguments():
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    buf = ctx.alloc(1 << 20)
    # zero frames: accepted, nothing launched
    assert L.mmw_range_doppler(h, buf.ptr, buf.ptr, None, 0, 12, 256, 128) == 0
    assert L.mmw_chain3d(h, buf.ptr, None, buf.ptr, 0, 12, 256, 128, 64, 0) == 0
    assert L.mmw_cfar2d(h, buf.ptr, None, None, buf.ptr, 0, 8, 8, 0, 1, 1, 0, 0, 1.0, 0) == 0
    # bad arguments -> MMW_ERR_INVALID (-1) with a message, surfaced as ValueError
    assert L.mmw_range_doppler(h, None, buf.ptr, None, 1, 12, 256, 128) == -1
    assert L.mmw_angle_fft(h, buf.ptr, buf.ptr, 1, 12, 8, 8, 8, 0) == -1          # A < V
    assert b"A >= V" in L.mmw_last_error()
    with pytest.raises(ValueError):
        _lib.check(L.mmw_cfar2d(h, buf.ptr, None, None, buf.ptr, 1, 8, 8, 1, 1, 1, 0, 0, 1.0, 99))   # k_rank > N
    with pytest.raises(ValueError):
        _lib.check(L.mmw_free(h, 12345))
    buf.free()
    # single antenna, single chirp-ish shapes through the Python API
    for shape in ((1, 8, 8), (2, 16, 2), (12, 4, 4), (3, 2, 5)):
        V, S, C = shape
        cm = make_cm(synth.synth_cfg_text(num_samples=S, num_loops=C))
        cube = synth.synth_cube(3, shape, num_targets=2)
        rd_got = RangeDopplerProcessor(cm).process(cube, rx_idx=-1, return_magnitude=False)
        rd_ref = O.range_doppler(cube)
        if np.max(np.abs(rd_ref)) > 0:  # hann(2) = [0, 0] zeroes the whole map in the reference too
            assert rel_err(rd_got, rd_ref) <= SPEC_TOL
        else:
            assert np.max(np.abs(rd_got)) == 0
        A = max(V, 4)
        got = RangeAngleProcessorDBSEnhanced(cm, num_angle_bins_range_angle_response=A).compute_3d_windowed_fft(cube)
        ref = O.fft3d_windowed(cube, A)
        if np.max(np.abs(ref)) > 0:     # hann(1) = 1, hann(2) = [0, 0]: the reference's own degenerate cases
            assert rel_err(got, ref) <= SPEC_TOL
        else:
            assert np.max(np.abs(got)) == 0
    with pytest.raises(ValueError):
        RangeDopplerProcessor(make_cm(synth.synth_cfg_text(8, 8))).process(np.zeros((8, 8), dtype=complex))


def test_doppler_azimuth_processor(golden):
    from mmwave_radar_processing_amd.processors import DopplerAzimuthProcessor
    g = golden("doppler_azimuth.npz")
    cm = make_cm(synth.synth_cfg_text(num_samples=32, num_loops=16))
    cube = synth.synth_cube(101, (12, 32, 16))
    p = DopplerAzimuthProcessor(cm, num_angle_bins=64)
    np.testing.assert_array_equal(p.valid_angle_bins, g["valid_angle_bins"])
    assert rel_err(p.process(cube), g["std_all"]) <= SPEC_TOL
    got = p.process(cube, rx_antennas=[4, 5, 8, 9], range_window=[0.9, 2.0], shift_angle=False, some_yaml_key=1)
    assert got.shape == g["std_sub_win"].shape and rel_err(got, g["std_sub_win"]) <= SPEC_TOL
    cm2 = ConfigManager()
    cm2.load_cfg_text(sample_cfg_text(), array_geometry="ods")
    p2 = DopplerAzimuthProcessor(cm2, num_angle_bins=64, valid_angle_range=[-1.04719755, 1.04719755])
    virt = synth.synth_cube(202, (12, 63, 70))
    got2 = p2.process(virt, rx_antennas=[4, 5, 8, 9], range_window=[0.9, 2.0], shift_angle=False)
    assert rel_err(got2, g["ods_sub"]) <= SPEC_TOL
    # headline shape against the oracle, both shift settings
    cm3 = make_cm(synth.SYNTH_CFG_256x128x12)
    sc3 = O.cfg_scalars(synth.SYNTH_CFG_256x128x12)
    c3 = synth.synth_cube(8)
    p3 = DopplerAzimuthProcessor(cm3)
    for shift in (True, False):
        ref = O.doppler_azimuth(c3, sc3, rx_antennas=[0, 3, 4, 7], range_window=[2.0, 9.0], shift_angle=shift)
        assert rel_err(p3.process(c3, rx_antennas=[0, 3, 4, 7], range_window=[2.0, 9.0], shift_angle=shift), ref) <= SPEC_TOL


def test_doppler_azimuth_precise_mode(golden):
    """use_precise_fft=True against the imported reference's outputs (scipy ZoomFFT inside) and, at the headline
    shape, against the oracle (reference: processors/doppler_azimuth_resp.py:130-294)."""
    from mmwave_radar_processing_amd.processors import DopplerAzimuthProcessor
    g = golden("doppler_azimuth.npz")
    cm = make_cm(synth.synth_cfg_text(num_samples=32, num_loops=16))
    cube = synth.synth_cube(101, (12, 32, 16))
    p = DopplerAzimuthProcessor(cm, num_angle_bins=64)
    for tag, vr, kw in (("default", [-0.25, 0.25], {}), ("pos_only", [0.3, 1.2], {}), ("narrow", [-0.05, 0.02], {}),
                        ("clamped", [-50.0, 50.0], {"shift_angle": False}),
                        ("neg_sub", [-1.0, -0.2], {"rx_antennas": [4, 5, 8, 9], "range_window": [0.9, 2.0]})):
        vr_in = np.array(vr)
        got = p.process(cube, use_precise_fft=True, precise_vel_range=vr_in, **kw)
        np.testing.assert_array_equal(vr_in, np.array(vr))               # the caller's array is not edited
        np.testing.assert_allclose(p.zoomed_vel_bins, g["precise_" + tag + "_bins"], rtol=0, atol=1e-15)
        assert got.shape == g["precise_" + tag].shape and got.dtype == np.float64
        assert rel_err(got, g["precise_" + tag]) <= SPEC_TOL, tag
    assert np.all(p.process(cube, use_precise_fft=True, precise_vel_range=[-0.05, 0.02])[:16] == 0)   # zero half
    cm2 = ConfigManager()
    cm2.load_cfg_text(sample_cfg_text(), array_geometry="ods")
    p2 = DopplerAzimuthProcessor(cm2, num_angle_bins=64, valid_angle_range=[-1.04719755, 1.04719755])
    virt = synth.synth_cube(202, (12, 63, 70))
    got2 = p2.process(virt, rx_antennas=[4, 5, 8, 9], range_window=[0.9, 2.0], use_precise_fft=True)
    np.testing.assert_allclose(p2.zoomed_vel_bins, g["precise_ods_bins"], rtol=0, atol=1e-15)
    assert rel_err(got2, g["precise_ods"]) <= SPEC_TOL
    cm3 = make_cm(synth.SYNTH_CFG_256x128x12)
    sc3 = O.cfg_scalars(synth.SYNTH_CFG_256x128x12)
    c3 = synth.synth_cube(8)
    p3 = DopplerAzimuthProcessor(cm3)
    for shift, vr in ((True, [-0.25, 0.25]), (False, [-1.5, 0.6])):
        ref, bins = O.doppler_azimuth_precise(c3, sc3, range_window=[2.0, 9.0], shift_angle=shift, vel_range=vr)
        got = p3.process(c3, range_window=[2.0, 9.0], shift_angle=shift, use_precise_fft=True, precise_vel_range=vr)
        np.testing.assert_allclose(p3.zoomed_vel_bins, bins, rtol=0, atol=1e-15)
        assert got.shape == (256, ref.shape[1]) and rel_err(got, ref) <= SPEC_TOL


def test_doppler_azimuth_zoom_batch_and_errors():
    """C entry on a batch of frames: frame f of the batch == the single-frame call; argument checks."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    F, V, S, C, A, M = 3, 8, 64, 32, 64, 40
    cubes = np.stack([synth.synth_cube(300 + f, (V, S, C)) for f in range(F)]).astype(np.complex64)
    freq = np.linspace(-0.2, 0.3, M)
    freq[5] = np.nan
    bufs = _lib.BufferSet(ctx)
    d_in = bufs.get("in", cubes.nbytes)
    d_in.upload(cubes)
    d_out = bufs.get("out", F * M * A * 4)
    fp = freq.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))
    _lib.check(L.mmw_doppler_azimuth_zoom(h, d_in.ptr, d_out.ptr, F, V, S, C, A, 3, 50, C - 2, fp, M, 0))
    batch = d_out.download((F, M, A), np.float32)
    assert np.all(batch[:, 5] == 0) and np.all(batch[:, 6] > 0)
    Z = np.exp(-2j * np.pi * np.outer(np.where(np.isnan(freq), 0, freq), np.arange(C - 2)))
    Z[5] = 0
    for f in range(F):
        x = cubes[f].astype(complex) * np.hanning(S)[None, :, None] * np.hanning(C)[None, None, :] * np.hanning(V)[:, None, None]
        r = np.fft.fft(x, axis=1)[:, 3:50, :C - 2]                       # [V, kept range, chirps used]
        y = np.einsum("kc,vsc->skv", Z, r)
        ref = np.mean(np.abs(np.fft.fftshift(np.fft.fft(y, n=A, axis=2), axes=2)), axis=0)
        assert rel_err(batch[f], ref) <= SPEC_TOL
    assert L.mmw_doppler_azimuth_zoom(h, d_in.ptr, d_out.ptr, F, V, S, C, A, 3, 50, C + 1, fp, M, 0) == _lib.MMW_ERR_INVALID
    assert L.mmw_doppler_azimuth_zoom(h, d_in.ptr, d_out.ptr, F, V, S, C, A, 10, 10, C, fp, M, 0) == _lib.MMW_ERR_INVALID
    assert L.mmw_doppler_azimuth_zoom(h, d_in.ptr, d_out.ptr, F, V, S, C, A, 0, S, C, fp, M, 1) == _lib.MMW_ERR_INVALID
    _lib.check(L.mmw_doppler_azimuth_zoom(h, d_in.ptr, d_out.ptr, 0, V, S, C, A, 0, S, C, fp, M, 0))
    bufs.free()


def test_processor_protocol_state_and_registries():
    """Plugin-host contract (reference: processors/_processor.py:6-64, view_controller.py:56-111)."""
    cm = make_cm(synth.synth_cfg_text(num_samples=32, num_loops=16))
    cube = synth.synth_cube(2, (12, 32, 16))
    params = {"cfar_type": "os_cfar_2d", "cfar_params": {"num_train": [2, 2], "num_guard": [1, 1], "rho": 0.7, "alpha": 3}}
    det = RangeDopplerDetector2D(cm, **params)
    dets = det.process(adc_cube=cube, **params)                 # ctor params re-passed to process()
    mag = np.abs(O.range_doppler(cube)[0])
    ref = O.os_cfar_2d(mag, (2, 2), (1, 1), 0.7, 3)[2]
    np.testing.assert_array_equal(dets, np.array(ref, dtype=np.int64).reshape(-1, 2))
    for key in ("range_bins", "vel_bins", "dets", "rng_dop_resp", "rng_dop_resp_raw"):
        assert isinstance(getattr(det, key), np.ndarray)
    assert det.detector.thresholds.shape == (32, 16) and det.detector.detections.dtype == bool
    det.update_history(estimated=np.array([1.0, 2.0]), ground_truth=np.array([1.5]))
    assert len(det.history_estimated) == 1 and len(det.history_gt) == 1
    det.reset()
    assert det.dets is None and det.rng_dop_resp is None and det.history_estimated == []
    r, v, ri, vi = det._map_detections_to_bins(np.empty((0, 2), dtype=int))
    assert r.size == 0 and vi.size == 0
    r, v, ri, vi = det._map_detections_to_bins(np.array([[3, 5], [7, 1]]))
    np.testing.assert_array_equal(r, det.range_bins[[3, 7]])
    np.testing.assert_array_equal(v, det.vel_bins[[5, 1]])
    reg = get_range_doppler_detector_registry()
    assert set(reg) == {"range_doppler_detector_2d", "range_doppler_detector_sequential", "range_doppler_ground_detector"}
    # a foreign magnitude map goes through the detector's own host path
    foreign = np.abs(np.random.default_rng(0).standard_normal((32, 16))) * 10
    out = det._detect(cube, foreign)
    np.testing.assert_array_equal(out, np.array(O.os_cfar_2d(foreign, (2, 2), (1, 1), 0.7, 3)[2], dtype=np.int64).reshape(-1, 2))
    # PointCloudGenerator with an empty frame
    pcg = PointCloudGenerator(cm, az_antenna_idxs=[0, 1, 2, 3], el_antenna_idxs=[],
                              detector_params={"cfar_type": "ca_cfar_2d", "cfar_params": CFAR})
    pc = pcg.process(np.zeros((12, 32, 16), dtype=complex))
    assert pc.shape == (0, 4)
    pcg.reset()


def test_generic_kernels_cover_the_headline_shape(monkeypatch):
    """The any-shape kernels (two-pass register FFT + LDS exchange) also handle 256x128, and every chain schedule
    gives the same result: fused and generic paths are cross-checked against each other and the oracle."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    F, V, S, C, A = 96, 12, 256, 128, 64
    n = V * S * C
    d_in, d_a, d_b = ctx.alloc(F * n * 8), ctx.alloc(F * A * S * C * 8), ctx.alloc(F * n * 8)
    _lib.check(L.mmw_synth_cubes(h, d_in.ptr, F, V, S, C, 4242, 8, 30.0))
    cubes = d_in.download((F, V, S, C), np.complex64)
    ref_rd = O.range_doppler(cubes[5])
    ref_3d = O.fft3d_windowed(cubes[95], A)
    results = []
    for env in ({}, {"MMW_NO_FUSED_RD": "1"}, {"MMW_NO_FUSED_ANGLE": "1"}, {"MMW_CHAIN_PIPELINE": "0"},
                {"MMW_NO_FUSED_RD": "1", "MMW_NO_FUSED_ANGLE": "1", "MMW_CHAIN_PIPELINE": "0"}):
        for k in ("MMW_NO_FUSED_RD", "MMW_NO_FUSED_ANGLE", "MMW_CHAIN_PIPELINE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d_a.zero()
        _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_a.ptr, F, V, S, C, A, 0))
        _lib.check(L.mmw_range_doppler(h, d_in.ptr, d_b.ptr, None, F, V, S, C))
        got_3d = d_a.download((A, S, C), np.complex64, 95 * A * S * C * 8)
        got_rd = d_b.download((V, S, C), np.complex64, 5 * n * 8)
        assert rel_err(got_3d, ref_3d) <= SPEC_TOL, env
        assert rel_err(got_rd, ref_rd) <= SPEC_TOL, env
        results.append(got_3d)
    assert rel_err(results[0], results[-1]) <= 2e-6
    # keeping the RD cube (d_rd given) takes the serial schedule and fills it
    _lib.check(L.mmw_chain3d(h, d_in.ptr, d_b.ptr, d_a.ptr, F, V, S, C, A, 0))
    assert rel_err(d_b.download((V, S, C), np.complex64, 5 * n * 8), ref_rd) <= SPEC_TOL
    for b in (d_in, d_a, d_b):
        b.free()


def test_range_zoom_fft(golden):
    g = golden("doppler_azimuth.npz")
    cm = make_cm(synth.synth_cfg_text(num_samples=32, num_loops=16))
    cube = synth.synth_cube(101, (12, 32, 16))
    z, zb = RangeProcessor(cm).zoom_fft(cube, range_start_m=0.6, range_stop_m=1.9, chirp_idx=3)
    assert rel_err(z, g["zoom_mag"]) <= SPEC_TOL
    np.testing.assert_array_equal(zb, g["zoom_bins"])
    cm2 = make_cm(synth.SYNTH_CFG_256x128x12)
    sc2 = O.cfg_scalars(synth.SYNTH_CFG_256x128x12)
    c2 = synth.synth_cube(6)
    z2, _ = RangeProcessor(cm2).zoom_fft(c2, 3.0, 7.5, chirp_idx=-1)
    assert rel_err(z2, O.range_zoom(c2, sc2, 3.0, 7.5, chirp_idx=-1)[0]) <= SPEC_TOL


def test_full_batch_size_independent_properties():
    """BASELINE full size (1250 resident frames per GPU, the configs[4] shard): properties that need no oracle.
    Parseval for the range-Doppler stage, linearity of the whole chain, a pure tone landing in its bin, and a
    checksum-of-checksums comparing the overlapped schedule against the serial one on every frame."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    F, V, S, C, A = 1250, 12, 256, 128, 64
    n = V * S * C
    d_in, d_rd, d_out = ctx.alloc(F * n * 8), ctx.alloc(F * n * 8), ctx.alloc(F * A * S * C * 8)
    _lib.check(L.mmw_synth_cubes(h, d_in.ptr, F, V, S, C, 20260, 8, 30.0))
    # ---- Parseval: sum |RD|^2 = S*C * sum |hann(S) hann(C) x|^2 per antenna plane
    _lib.check(L.mmw_range_doppler(h, d_in.ptr, d_rd.ptr, None, F, V, S, C))
    win = np.hanning(S)[:, None] * np.hanning(C)[None, :]
    for f in (0, 417, 1249):
        x = d_in.download((V, S, C), np.complex64, f * n * 8).astype(np.complex128)
        rd = d_rd.download((V, S, C), np.complex64, f * n * 8).astype(np.complex128)
        lhs = np.sum(np.abs(rd) ** 2, axis=(1, 2))
        rhs = S * C * np.sum(np.abs(x * win) ** 2, axis=(1, 2))
        np.testing.assert_allclose(lhs, rhs, rtol=2e-6)
    # ---- linearity of the full chain on frames of the batch: chain(2x - 3j y) = 2 chain(x) - 3j chain(y)
    _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_out.ptr, F, V, S, C, A, 0))
    fx, fy = 100, 1100
    x = d_in.download((V, S, C), np.complex64, fx * n * 8)
    y = d_in.download((V, S, C), np.complex64, fy * n * 8)
    cx = d_out.download((A, S, C), np.complex64, fx * A * S * C * 8).astype(np.complex128)
    cy = d_out.download((A, S, C), np.complex64, fy * A * S * C * 8).astype(np.complex128)
    mix = (2.0 * x - 3.0j * y).astype(np.complex64)
    d_mix, d_mix_out = ctx.alloc(n * 8), ctx.alloc(A * S * C * 8)
    d_mix.upload(mix)
    _lib.check(L.mmw_chain3d(h, d_mix.ptr, None, d_mix_out.ptr, 1, V, S, C, A, 0))
    cm_ = d_mix_out.download((A, S, C), np.complex64).astype(np.complex128)
    expect = 2.0 * cx - 3.0j * cy
    assert np.max(np.abs(cm_ - expect)) / np.max(np.abs(expect)) <= 1e-6
    # ---- a pure tone lands in its (angle, range, Doppler) bin: x = exp(j 2 pi (kr s/S + kc c/C + ka v/A))
    kr, kc, ka = 37, -21, 9
    v_, s_, c_ = np.meshgrid(np.arange(V), np.arange(S), np.arange(C), indexing="ij")
    tone = (1000.0 * np.exp(2j * np.pi * (kr * s_ / S + kc * c_ / C + ka * v_ / A))).astype(np.complex64)
    d_mix.upload(tone)
    _lib.check(L.mmw_chain3d(h, d_mix.ptr, None, d_mix_out.ptr, 1, V, S, C, A, 0))
    mag = np.abs(d_mix_out.download((A, S, C), np.complex64))
    assert np.unravel_index(np.argmax(mag), mag.shape) == ((ka + A // 2) % A, kr, (kc + C // 2) % C)
    # ---- checksum of checksums: serial schedule vs overlapped schedule, all 1250 frames
    os.environ["MMW_CHAIN_PIPELINE"] = "0"
    try:
        d_out2 = ctx.alloc(F * A * S * C * 4)
        d_out1 = ctx.alloc(F * A * S * C * 4)
        _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_out2.ptr, F, V, S, C, A, 1))     # serial, |.| output
    finally:
        del os.environ["MMW_CHAIN_PIPELINE"]
    _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_out1.ptr, F, V, S, C, A, 1))         # overlapped
    sums1 = np.empty(F)
    sums2 = np.empty(F)
    step = 50
    for f0 in range(0, F, step):
        a = d_out1.download((step, A * S * C), np.float32, f0 * A * S * C * 4)
        b = d_out2.download((step, A * S * C), np.float32, f0 * A * S * C * 4)
        sums1[f0:f0 + step] = a.sum(axis=1, dtype=np.float64)
        sums2[f0:f0 + step] = b.sum(axis=1, dtype=np.float64)
        # same arithmetic in separately compiled kernels (the compiler contracts a few multiply-adds differently):
        # a few units in the last place of float32, far inside the 1e-5 budget
        assert cross_schedule_dev(a[::7], b[::7]) <= CROSS_SCHEDULE_TOL
    np.testing.assert_allclose(sums1, sums2, rtol=1e-7)
    assert np.all(sums1 > 0)
    for b_ in (d_in, d_rd, d_out, d_mix, d_mix_out, d_out1, d_out2):
        b_.free()


def test_chain_schedules_agree_and_hand_over(monkeypatch):
    """mmw_chain3d has three schedules for the 256 x 128 plane: serial, overlapped with events per chunk of frames, and
    device-synchronised (one range-Doppler and one angle launch per call, frames handed over through counters and a
    ring in device memory).  They run the same arithmetic in separately compiled kernels: outputs agree to float32
    rounding across schedules and are bit-identical within one schedule -- for batches shorter and longer than the ring,
    back to back without a host sync, and across a change of the ring layout."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    S, C, A = 256, 128, 64
    F = 130
    d_in = ctx.alloc(F * 12 * S * C * 8)
    d_out = ctx.alloc(F * A * S * C * 8)
    d_out2 = ctx.alloc(F * A * S * C * 8)
    _lib.check(L.mmw_synth_cubes(h, d_in.ptr, F, 12, S, C, 4242, 8, 30.0))

    def run(mode, n_frames, V, out, flags=0):
        monkeypatch.setenv("MMW_CHAIN_PIPELINE", "0" if mode == "serial" else "1")
        monkeypatch.setenv("MMW_CHAIN_MODE", "events" if mode == "events" else "sync")
        plan = (_lib.C.c_int * 8)()
        _lib.check(L.mmw_diag_chain_plan(h, n_frames, V, S, C, A, flags, plan))
        assert (bool(plan[0]), bool(plan[6])) == {"serial": (False, False), "events": (True, False),
                                                  "sync": (True, True)}[mode]
        _lib.check(L.mmw_chain3d(h, d_in.ptr, None, out.ptr, n_frames, V, S, C, A, flags))

    def fetch(out, n_frames, esz=8):
        return out.download((n_frames, A, S, C), np.complex64 if esz == 8 else np.float32)

    run("serial", F, 12, d_out)
    ref = fetch(d_out, F)
    cube0 = d_in.download((12, S, C), np.complex64)
    assert rel_err(ref[0], O.fft3d_windowed(cube0, A)) <= SPEC_TOL
    for mode in ("events", "sync"):
        d_out.zero()
        run(mode, F, 12, d_out)
        got = fetch(d_out, F)
        print(f"schedule {mode} vs serial: max deviation {cross_schedule_dev(got, ref):.2e} of the peak, "
              f"bit-identical: {np.array_equal(got, ref)}")
        assert cross_schedule_dev(got, ref) <= CROSS_SCHEDULE_TOL, mode
        if mode == "sync":
            ref_sync = got
    # device-synchronised: batches shorter than the ring, back to back into two buffers, no host sync in between
    d_out.zero()
    d_out2.zero()
    run("sync", 5, 12, d_out)
    run("sync", 77, 12, d_out2)
    run("sync", 3, 12, d_out)           # overwrites the first three frames of the 5-frame result with the same values
    assert np.array_equal(fetch(d_out, 5), ref_sync[:5])        # one schedule: bit-identical whatever the batch
    assert np.array_equal(fetch(d_out2, 77), ref_sync[:77])
    # change of layout with work in flight: the same bytes read as 8-antenna cubes (no end-plane skipping there: the
    # Hann(8) end points are zero as well, so V = 8 skips too), magnitude output, then back to 12 antennas
    F8 = F * 12 // 8
    run("sync", F8, 8, d_out2, 1)
    ref8 = fetch(d_out2, F8, 4)[:100].copy()
    run("serial", 100, 8, d_out2, 1)
    assert cross_schedule_dev(fetch(d_out2, 100, 4), ref8) <= CROSS_SCHEDULE_TOL
    d_out2.zero()
    run("sync", F, 12, d_out)
    run("sync", 100, 8, d_out2, 1)
    run("events", 40, 12, d_out)
    run("sync", F, 12, d_out)
    assert np.array_equal(fetch(d_out2, 100, 4), ref8)
    assert np.array_equal(fetch(d_out, F), ref_sync)
    for b in (d_in, d_out, d_out2):
        b.free()


def test_overlapped_chain_on_an_lds_resident_shape():
    """12x64x64 cubes (k_rd_lds + k_angle64): batch large enough for the overlapped schedule (chunk ~ 330 frames)."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    F, V, S, C, A = 1500, 12, 64, 64, 64
    n = V * S * C
    d_in, d_out = ctx.alloc(F * n * 8), ctx.alloc(F * A * S * C * 8)
    _lib.check(L.mmw_synth_cubes(h, d_in.ptr, F, V, S, C, 99, 6, 30.0))
    for _ in range(2):
        _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_out.ptr, F, V, S, C, A, 0))
    for f in (0, 331, 332, 333, 665, 666, 1000, 1499):
        cube = d_in.download((V, S, C), np.complex64, f * n * 8)
        got = d_out.download((A, S, C), np.complex64, f * A * S * C * 8)
        assert rel_err(got, O.fft3d_windowed(cube, A)) <= SPEC_TOL, f
    d_in.free()
    d_out.free()


# every (samples, loops) plane of the cfg files the reference ships (tests/golden/cfg_scalars.json), plus a few more
# factorisations: prime axis, radix-32 class, single-level axes, odd cell count
MIXED_SHAPES = [(200, 40), (254, 50), (130, 50), (100, 30), (63, 115), (90, 100), (90, 80), (63, 100), (63, 127),
                (127, 32), (63, 70), (70, 40), (512, 32), (64, 40), (100, 100), (120, 126), (512, 8),
                (13, 11), (96, 23), (25, 49), (7, 3), (1, 6), (16, 1), (37, 41), (74, 10), (1024, 8)]


@pytest.mark.parametrize("S,C", MIXED_SHAPES)
def test_mixed_radix_rd_kernel_all_shipped_shapes(S, C, monkeypatch):
    """LDS-resident mixed-radix RD kernel (mmw_fft_mixed.h): spectrum against the oracle and against the generic
    two-kernel path, float64 CFAR plane, and bit-exact CA-CFAR detections from it."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    F, V = 3, 4
    n = V * S * C
    cubes = np.stack([synth.synth_cube(7000 + 13 * S + C + f, (V, S, C)) for f in range(F)]).astype(np.complex64)
    d_in, d_rd, d_mag = ctx.alloc(F * n * 8), ctx.alloc(F * n * 8), ctx.alloc(F * S * C * 8)
    d_in.upload(cubes)
    got = {}
    for no_mixed in ("0", "1"):
        monkeypatch.setenv("MMW_NO_MIXED_RD", no_mixed)
        d_rd.zero()
        d_mag.zero()
        _lib.check(L.mmw_range_doppler(h, d_in.ptr, d_rd.ptr, None, F, V, S, C))
        _lib.check(L.mmw_range_doppler_mag64(h, d_in.ptr, d_mag.ptr, F, V, S, C, 1))
        got[no_mixed] = (d_rd.download((F, V, S, C), np.complex64), d_mag.download((F, S, C), np.float64))
    monkeypatch.delenv("MMW_NO_MIXED_RD")
    for f in range(F):
        ref = O.range_doppler(cubes[f])
        for key in ("0", "1"):
            assert rel_err(got[key][0][f], ref) <= SPEC_TOL, key
            assert rel_err(got[key][1][f], np.abs(ref[1])) <= 1e-12, key
    if S >= 13 and C >= 13:
        det = CaCFAR2D(num_train=(2, 2), num_guard=(1, 1), pfa=1e-3)
        for f in range(F):
            ref_mag = np.abs(O.range_doppler(cubes[f])[1])
            want = O.ca_cfar_2d(ref_mag, (2, 2), (1, 1), 1e-3)[2]
            have = det.detect(got["0"][1][f])
            np.testing.assert_array_equal(np.asarray(have).reshape(-1, 2), np.array(want, dtype=np.int64).reshape(-1, 2))
    for b in (d_in, d_rd, d_mag):
        b.free()


@pytest.mark.parametrize("S,C", [(63, 127), (127, 32), (254, 50)])
def test_both_forms_of_the_127_point_level_meet_the_oracle(S, C):
    """The 127-point DFT level of the shipped 63x127 / 127x32 / 254x50 planes has two forms: float32 MFMAs and the exact
    three-way bfloat16 split (MMW_BIGPRIME_BF16, the default where it fits).  Both against the oracle at the 1e-5 bar, stand-alone
    and as the producer of the device-synchronised chain, and against each other to float32 rounding."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    F, V, A = 40, 12, 64
    n = V * S * C
    cubes = np.stack([synth.synth_cube(9100 + S + C + f, (V, S, C)) for f in range(F)]).astype(np.complex64)
    d_in, d_rd, d_out = ctx.alloc(F * n * 8), ctx.alloc(F * n * 8), ctx.alloc(F * A * S * C * 8)
    d_in.upload(cubes)
    rd, ch = {}, {}
    try:
        for form in (0, 1):
            ctx.set_option("MMW_BIGPRIME_BF16", form)
            ctx.set_option("MMW_CHAIN_PIPELINE", 1)
            d_rd.zero()
            d_out.zero()
            _lib.check(L.mmw_range_doppler(h, d_in.ptr, d_rd.ptr, None, F, V, S, C))
            _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_out.ptr, F, V, S, C, A, 0))
            rd[form] = d_rd.download((F, V, S, C), np.complex64)
            ch[form] = d_out.download((F, A, S, C), np.complex64)
    finally:
        ctx.set_option("MMW_BIGPRIME_BF16", None)
        ctx.set_option("MMW_CHAIN_PIPELINE", None)
    for f in (0, F // 2, F - 1):
        ref_rd, ref_ch = O.range_doppler(cubes[f]), O.fft3d_windowed(cubes[f], A)
        for form in (0, 1):
            assert rel_err(rd[form][f], ref_rd) <= SPEC_TOL, (form, f)
            assert rel_err(ch[form][f], ref_ch) <= SPEC_TOL, (form, f)
    dev_rd, dev_ch = cross_schedule_dev(rd[1], rd[0]), cross_schedule_dev(ch[1], ch[0])
    print(f"127-point level {S}x{C}: bfloat16 x 3 against float32 MFMAs: RD {dev_rd:.2e}, chain {dev_ch:.2e} of the peak")
    assert max(dev_rd, dev_ch) <= CROSS_SCHEDULE_TOL
    for b in (d_in, d_rd, d_out):
        b.free()


@pytest.mark.parametrize("nrx,ntx,S,C", [(4, 3, 256, 128), (4, 3, 64, 32), (4, 3, 63, 70), (4, 2, 100, 30), (2, 2, 512, 64),
                                         (4, 3, 63, 127), (2, 2, 256, 256)])
def test_raw_cube_entry_points_fold_the_virtual_array_reformat(nrx, ntx, S, C):
    """mmw_range_doppler_raw / mmw_chain3d_raw == mmw_virtual_array_reformat followed by the plain calls, on the
    fused 256x128 kernel, an LDS-resident power-of-two plane, mixed-radix planes and the two-kernel fallback; and
    against the oracle (virtual_array_reformater.py:53-63 + range_doppler_resp.py:94-103)."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    F, V, A = 5, nrx * ntx, 64
    rng = np.random.default_rng(S * 1000 + C)
    raw = (rng.integers(-500, 500, (F, nrx, S, ntx * C)) + 1j * rng.integers(-500, 500, (F, nrx, S, ntx * C))).astype(np.complex64)
    n = V * S * C
    d_raw, d_virt, d_a, d_b = ctx.alloc(F * n * 8), ctx.alloc(F * n * 8), ctx.alloc(F * n * 8), ctx.alloc(F * n * 8)
    d_3a, d_3b = ctx.alloc(F * A * S * C * 8), ctx.alloc(F * A * S * C * 8)
    d_raw.upload(raw)
    _lib.check(L.mmw_virtual_array_reformat(h, d_raw.ptr, d_virt.ptr, F, nrx, ntx, S, C))
    _lib.check(L.mmw_range_doppler(h, d_virt.ptr, d_a.ptr, None, F, V, S, C))
    _lib.check(L.mmw_range_doppler_raw(h, d_raw.ptr, d_b.ptr, F, nrx, ntx, S, C))
    rd_a, rd_b = d_a.download((F, V, S, C), np.complex64), d_b.download((F, V, S, C), np.complex64)
    np.testing.assert_array_equal(rd_a, rd_b)                       # same arithmetic, only the load addresses differ
    d_a.zero()
    _lib.check(L.mmw_chain3d(h, d_virt.ptr, None, d_3a.ptr, F, V, S, C, A, 0))
    _lib.check(L.mmw_chain3d_raw(h, d_raw.ptr, d_a.ptr, d_3b.ptr, F, nrx, ntx, S, C, A, 0))
    np.testing.assert_array_equal(d_3a.download((F, A, S, C), np.complex64), d_3b.download((F, A, S, C), np.complex64))
    np.testing.assert_array_equal(d_a.download((F, V, S, C), np.complex64), rd_b)      # kept RD cube
    virt = O.virtual_array_reformat(raw[F - 1], nrx, 0, ntx - 1, C)
    assert rel_err(rd_b[F - 1], O.range_doppler(virt)) <= SPEC_TOL
    assert L.mmw_range_doppler_raw(h, d_raw.ptr, d_b.ptr, F, 0, ntx, S, C) == _lib.MMW_ERR_INVALID
    for b in (d_raw, d_virt, d_a, d_b, d_3a, d_3b):
        b.free()


def test_frame_pipeline_from_raw_cubes():
    """FramePipeline.load_raw / chain3d_raw against the host-side VirtualArrayReformatter + per-frame processor."""
    from mmwave_radar_processing_amd.batch import FramePipeline
    from mmwave_radar_processing_amd.processors import VirtualArrayReformatter
    cm = make_cm(synth.synth_cfg_text(num_samples=64, num_loops=32))
    F, nrx, ntx, S, C = 4, 4, 3, 64, 32
    rng = np.random.default_rng(77)
    raw = (rng.integers(-300, 300, (F, nrx, S, ntx * C)) + 1j * rng.integers(-300, 300, (F, nrx, S, ntx * C))).astype(np.complex64)
    pipe = FramePipeline(cm, max_frames=F, shape=(nrx * ntx, S, C))
    pipe.load_raw(raw, ntx)
    ref_virt = np.stack([VirtualArrayReformatter(cm).process(raw[f]) for f in range(F)])
    np.testing.assert_array_equal(pipe.cubes(), ref_virt.astype(np.complex64))
    pipe.chain3d_raw()
    got = pipe.fetch_chain3d(F - 1)
    assert rel_err(got, O.fft3d_windowed(ref_virt[F - 1], 64)) <= SPEC_TOL
    pipe.chain3d()
    np.testing.assert_array_equal(pipe.fetch_chain3d(F - 1), got)
    with pytest.raises(ValueError):
        pipe.load_raw(raw, 5)


def test_subclass_in_the_style_of_velocity_estimator():
    """A processor derived from DopplerAzimuthProcessor the way the reference's VelocityEstimator is
    (velocity_estimator.py:7,48-51,175-199,278-299): super().__init__(config_manager=..., ...), super().process(...),
    self.detect_peaks_rows(...), reset() -- works unchanged on the drop-in base class."""
    from mmwave_radar_processing_amd.processors import DopplerAzimuthProcessor

    class Est(DopplerAzimuthProcessor):
        def __init__(self, config_manager, precise_vel_bound=0.25, **kwargs):
            super().__init__(config_manager=config_manager, num_angle_bins=64,
                             valid_angle_range=np.array([np.deg2rad(-70), np.deg2rad(70)]))
            self.precise_vel_bound = precise_vel_bound
            self.azimuth_peaks = None

        def process(self, adc_cube, **kwargs):
            resp = super().process(adc_cube=adc_cube, rx_antennas=[0, 1, 2, 3, 4, 5, 6, 7], range_window=[1.0, 12.0],
                                   use_precise_fft=True,
                                   precise_vel_range=np.array([-self.precise_vel_bound, self.precise_vel_bound]))
            self.azimuth_peaks = self.detect_peaks_rows(resp, vel_bins=self.zoomed_vel_bins, min_threshold_dB=30.0)
            return resp

    cm = make_cm(synth.SYNTH_CFG_256x128x12)
    sc = O.cfg_scalars(synth.SYNTH_CFG_256x128x12)
    cube = synth.synth_cube(12)
    est = Est(cm)
    resp = est.process(cube)
    ref, bins = O.doppler_azimuth_precise(cube, sc, rx_antennas=list(range(8)), range_window=[1.0, 12.0],
                                          vel_range=[-0.25, 0.25], valid_angle_range=(np.deg2rad(-70), np.deg2rad(70)))
    assert rel_err(resp, ref) <= SPEC_TOL
    want = est.detect_peaks_rows(ref, vel_bins=bins, min_threshold_dB=30.0)      # same picker on the float64 map
    assert est.azimuth_peaks.shape == want.shape and want.shape[0] > 0
    np.testing.assert_array_equal(est.azimuth_peaks[:, 1], want[:, 1])
    assert np.max(np.abs(est.azimuth_peaks[:, 0] - want[:, 0])) <= 0.06              # at most one angle bin apart
    est.reset()


@pytest.mark.parametrize("V,S,C,A,win", [(12, 256, 128, 64, (0, 256)), (8, 64, 32, 64, (5, 41)), (4, 63, 70, 64, (0, 63)),
                                         (12, 63, 100, 64, (10, 11)), (5, 32, 16, 32, (0, 32)), (12, 31, 15, 64, (3, 30))])
def test_doppler_azimuth_entry_fused_range_mean(V, S, C, A, win, monkeypatch):
    """mmw_doppler_azimuth (RD kernel + fused angle FFT / |.| / range mean) == mmw_chain3d(MAGNITUDE) +
    mmw_mean_over_range == the oracle's coarse Doppler-azimuth map, for batches whose last chunk is short too."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    F = 7
    cubes = np.stack([synth.synth_cube(4100 + f, (V, S, C)) for f in range(F)]).astype(np.complex64)
    d_in, d_mag = ctx.alloc(cubes.nbytes), ctx.alloc(F * A * S * C * 4)
    d_a, d_b = ctx.alloc(F * C * A * 4), ctx.alloc(F * C * A * 4)
    d_in.upload(cubes)
    lo, hi = win
    for flags in (0, _lib.ANGLE_NO_SHIFT, _lib.ANGLE_NO_WINDOW):
        _lib.check(L.mmw_doppler_azimuth(h, d_in.ptr, d_a.ptr, F, V, S, C, A, lo, hi, flags))
        _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_mag.ptr, F, V, S, C, A, flags | _lib.ANGLE_MAGNITUDE))
        _lib.check(L.mmw_mean_over_range(h, d_mag.ptr, d_b.ptr, F, A, S, C, lo, hi))
        got, two_pass = d_a.download((F, C, A), np.float32), d_b.download((F, C, A), np.float32)
        assert rel_err(got, two_pass) <= 2e-6, flags
        for f in (0, F - 1):
            x = cubes[f].astype(complex) * np.hanning(S)[None, :, None] * np.hanning(C)[None, None, :]
            rd = np.fft.fftshift(np.fft.fft2(x, axes=(1, 2)), axes=2)
            if not flags & _lib.ANGLE_NO_WINDOW:
                rd = rd * np.hanning(V)[:, None, None]
            ang = np.fft.fft(rd, n=A, axis=0)
            if not flags & _lib.ANGLE_NO_SHIFT:
                ang = np.fft.fftshift(ang, axes=0)
            ref = np.mean(np.abs(ang[:, lo:hi, :]), axis=1).T                    # [C][A]
            assert rel_err(got[f], ref) <= SPEC_TOL, (flags, f)
    monkeypatch.setenv("MMW_NO_FUSED_ANGLE", "1")                               # unfused tail inside the same entry
    _lib.check(L.mmw_doppler_azimuth(h, d_in.ptr, d_b.ptr, F, V, S, C, A, lo, hi, _lib.ANGLE_NO_WINDOW))
    assert rel_err(d_b.download((F, C, A), np.float32), got) <= 2e-6
    assert L.mmw_doppler_azimuth(h, d_in.ptr, d_a.ptr, F, V, S, C, A, hi, hi, 0) == _lib.MMW_ERR_INVALID
    assert L.mmw_doppler_azimuth(h, d_in.ptr, d_a.ptr, F, V, S, C, A, lo, hi, 1) == _lib.MMW_ERR_INVALID
    for b in (d_in, d_mag, d_a, d_b):
        b.free()


@pytest.mark.parametrize("V,S,C", [(12, 63, 100), (8, 21, 10), (4, 25, 26), (12, 2, 5), (16, 7, 18), (12, 127, 2),
                                   (12, 63, 127), (8, 21, 11), (4, 5, 5), (16, 1, 1), (12, 9, 25), (12, 3, 37),
                                   (12, 90, 100), (8, 13, 24), (4, 3, 4), (12, 7, 40)])
@pytest.mark.parametrize("flags", [0, _lib.ANGLE_NO_WINDOW | _lib.ANGLE_NO_SHIFT, _lib.ANGLE_MAGNITUDE])
def test_angle_rows_kernel_on_misaligned_rows(V, S, C, flags):
    """k_angle64_rows / k_angle64_rows_odd (bins % 16 != 0: every wave stores a per-row line-aligned window of the cells it computed) against
    numpy's FFT over the antenna axis (range_angle_resp_dbs_enhanced.py:175-196), several frames so that the frame
    stride, the first / last wave of a row and rows with every misalignment (a * bins mod 16) are hit."""
    ctx = _lib.default_context()
    F, A, bins = 3, 64, S * C
    assert bins % 16 != 0                   # odd bin counts: k_angle64_rows_odd (complex output only: generic kernel for |.|)
    rng = np.random.default_rng(V * 1000 + bins)
    rd = (rng.standard_normal((F, V, S, C)) + 1j * rng.standard_normal((F, V, S, C))).astype(np.complex64)
    mag = bool(flags & _lib.ANGLE_MAGNITUDE)
    esz = 4 if mag else 8
    d_rd, d_out = ctx.alloc(rd.nbytes), ctx.alloc(F * A * bins * esz + 256)
    d_rd.upload(rd)
    guard = np.full(32, 7.0 + 7.0j, np.complex64)           # nothing may be written past the last row
    d_out.upload(guard, byte_offset=F * A * bins * esz)
    _lib.check(ctx.lib.mmw_angle_fft(ctx.handle, d_rd.ptr, d_out.ptr, F, V, S, C, A, flags))
    got = d_out.download((F, A, S, C), np.float32 if mag else np.complex64)
    np.testing.assert_array_equal(d_out.download((32,), np.complex64, byte_offset=F * A * bins * esz), guard)
    x = rd.astype(np.complex128)
    if not flags & _lib.ANGLE_NO_WINDOW:
        x = x * np.hanning(V)[None, :, None, None]
    ref = np.fft.fft(x, n=A, axis=1)
    if not flags & _lib.ANGLE_NO_SHIFT:
        ref = np.fft.fftshift(ref, axes=1)
    if mag:
        ref = np.abs(ref)
    assert rel_err(got, ref) <= SPEC_TOL
    d_rd.free()
    d_out.free()


@pytest.mark.parametrize("V,S,C,n_used,kind", [(4, 32, 128, 128, "two_halves"), (4, 16, 64, 50, "long_run"), (4, 8, 320, 300, "l1024"),
                                               (4, 16, 40, 40, "irregular"), (4, 16, 128, 127, "nan_runs")])
def test_zoom_chirpz_against_direct_form(V, S, C, n_used, kind):
    """mmw_doppler_azimuth_zoom evaluates the zoom transform by chirp-z (mmw_czt.h: uniform runs of the frequency list,
    256- or 1024-point convolutions); MMW_ZOOM_DIRECT=1 keeps the direct n_used x M table of round 1.  Both against the
    float64 sum, on lists that exercise run splitting, single-bin runs, NaN (zero-filled) bins and both FFT lengths."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    F, A = 2, 64
    rng = np.random.default_rng(len(kind) * 100 + n_used)
    if kind == "two_halves":
        freq = np.concatenate((np.linspace(0.974, 1.0, 128, endpoint=False), np.linspace(0.0, 0.026, 128, endpoint=False)))
    elif kind == "long_run":
        freq = np.linspace(-0.3, 0.4, 500)                  # one run, split into pieces of 256 - 50 + 1 bins
    elif kind == "l1024":
        freq = np.linspace(0.1, 0.2, 200, endpoint=False)
    elif kind == "irregular":
        freq = np.sort(rng.uniform(-0.5, 0.5, 24))          # no two spacings equal: 2-bin and 1-bin runs
    else:
        freq = np.linspace(-0.1, 0.1, 90)
        freq[:7] = np.nan
        freq[40:43] = np.nan
        freq[-1] = np.nan
    M = freq.size
    cubes = np.stack([synth.synth_cube(900 + f, (V, S, C)) for f in range(F)]).astype(np.complex64)
    bufs = _lib.BufferSet(ctx)
    d_in = bufs.get("in", cubes.nbytes)
    d_in.upload(cubes)
    d_out = bufs.get("out", F * M * A * 4)
    fp = freq.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))
    outs = {}
    for mode in ("czt", "direct"):
        if mode == "direct":
            os.environ["MMW_ZOOM_DIRECT"] = "1"
        try:
            _lib.check(L.mmw_doppler_azimuth_zoom(h, d_in.ptr, d_out.ptr, F, V, S, C, A, 1, S - 2, n_used, fp, M, 0))
        finally:
            os.environ.pop("MMW_ZOOM_DIRECT", None)
        outs[mode] = d_out.download((F, M, A), np.float32)
    nan = np.isnan(freq)
    Z = np.exp(-2j * np.pi * np.outer(np.where(nan, 0, freq), np.arange(n_used)))
    Z[nan] = 0
    for f in range(F):
        x = cubes[f].astype(complex) * np.hanning(S)[None, :, None] * np.hanning(C)[None, None, :] * np.hanning(V)[:, None, None]
        r = np.fft.fft(x, axis=1)[:, 1:S - 2, :n_used]
        y = np.einsum("kc,vsc->skv", Z, r)
        ref = np.mean(np.abs(np.fft.fftshift(np.fft.fft(y, n=A, axis=2), axes=2)), axis=0)
        for mode in outs:
            assert rel_err(outs[mode][f], ref) <= SPEC_TOL, mode
        assert np.all(outs["czt"][f][nan] == 0)
    bufs.free()


def test_range_zoom_chirpz_against_float64_sum():
    """mmw_range_zoom: 256 samples -> 1024-point chirp-z against the float64 direct sum (range_resp.py:59-102)."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    F, V, S, C, m = 2, 12, 256, 16, 300
    cubes = np.stack([synth.synth_cube(70 + f, (V, S, C)) for f in range(F)]).astype(np.complex64)
    d_in, d_out = ctx.alloc(cubes.nbytes), ctx.alloc(F * m * 4)
    d_in.upload(cubes)
    f0, df = 0.0123, 0.0007
    outs = {}
    for mode in ("czt", "direct"):
        if mode == "direct":
            os.environ["MMW_ZOOM_DIRECT"] = "1"
        try:
            _lib.check(L.mmw_range_zoom(h, d_in.ptr, d_out.ptr, F, V, S, C, 5, m, f0, df))
        finally:
            os.environ.pop("MMW_ZOOM_DIRECT", None)
        outs[mode] = d_out.download((F, m), np.float32)
    Z = np.exp(-2j * np.pi * np.outer(f0 + df * np.arange(m), np.arange(S)))
    for f in range(F):
        x = cubes[f][:, :, 5].astype(complex) * np.hanning(S)[None, :]
        ref = np.mean(np.abs(x @ Z.T), axis=0)
        for mode in outs:
            assert rel_err(outs[mode][f], ref) <= SPEC_TOL, mode
    d_in.free()
    d_out.free()


@pytest.mark.parametrize("S,C,F,V", [(63, 100, 700, 12), (254, 50, 150, 12), (64, 40, 900, 12), (63, 127, 200, 12), (100, 100, 300, 12),
                                     (63, 115, 160, 12), (127, 32, 900, 4), (63, 70, 500, 8), (32, 32, 2000, 16)])
def test_device_synchronised_chain_on_shipped_cfg_shapes(monkeypatch, S, C, F, V):
    """The device-synchronised chain with the compile-time mixed-radix range-Doppler producer (k_rd_mixed_ct MODE 2) and,
    where the angle rows are not line aligned, the row-window consumer (k_angle64_sync ROWS): serial vs events vs sync
    agree to float32 rounding, sync is bit-identical with itself for any batch length, frame 0 / last match the oracle.
    63 x 127 and 63 x 115 have odd bin counts: per-cell ring reads and shifted pairs in the consumer (ROWS 2)."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    A = 64
    d_in = ctx.alloc(F * V * S * C * 8)
    d_out = ctx.alloc(F * A * S * C * 8)
    _lib.check(L.mmw_synth_cubes(h, d_in.ptr, F, V, S, C, 777, 6, 30.0))

    def run(mode, n_frames, out):
        monkeypatch.setenv("MMW_CHAIN_PIPELINE", "0" if mode == "serial" else "1")
        monkeypatch.setenv("MMW_CHAIN_MODE", "events" if mode == "events" else "sync")
        plan = (_lib.C.c_int * 8)()
        _lib.check(L.mmw_diag_chain_plan(h, n_frames, V, S, C, A, 0, plan))
        _lib.check(L.mmw_chain3d(h, d_in.ptr, None, out.ptr, n_frames, V, S, C, A, 0))
        return bool(plan[0]), bool(plan[6])

    run("serial", F, d_out)
    ref = d_out.download((F, A, S, C), np.complex64)
    for f in (0, F - 1):
        cube = d_in.download((V, S, C), np.complex64, byte_offset=f * V * S * C * 8)
        assert rel_err(ref[f], O.fft3d_windowed(cube, A)) <= SPEC_TOL
    d_out.zero()
    assert run("sync", F, d_out) == (True, True)
    got = d_out.download((F, A, S, C), np.complex64)
    assert cross_schedule_dev(got, ref) <= CROSS_SCHEDULE_TOL
    if True:
        d_out.zero()
        run("sync", 7, d_out)               # shorter than the ring, straight after the long call
        run("sync", F // 3, d_out)
        np.testing.assert_array_equal(d_out.download((F // 3, A, S, C), np.complex64), got[:F // 3])
        d_out.zero()
        assert run("events", F, d_out) == (True, False)
        assert cross_schedule_dev(d_out.download((F, A, S, C), np.complex64), ref) <= CROSS_SCHEDULE_TOL
        run("sync", F, d_out)
        np.testing.assert_array_equal(d_out.download((F, A, S, C), np.complex64), got)
    d_in.free()
    d_out.free()


@pytest.mark.parametrize("S,C", [(512, 64), (128, 256), (1024, 32), (256, 256), (512, 128)])
def test_split_range_doppler_kernel_for_planes_beyond_the_lds(S, C, monkeypatch):
    """k_rd_split2_ct: planes of 2 x 16384 cells in ONE pass over HBM (even chirps through the LDS, odd chirps and then the
    even half's spectrum carried in registers, radix-2 combine in the store pass) against the oracle and the two-kernel
    path, and through the chain (Hann(V) end planes skipped there).  k_rd_split4_ct: planes of 4 x 16384 cells (256 x 256,
    512 x 128) -- four quarters of sample rows through the LDS, three of their spectra carried in registers, radix-4 combine
    in the store pass."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    F, V, A = 3, 4, 64
    n = V * S * C
    cubes = np.stack([synth.synth_cube(4100 + S + C + f, (V, S, C)) for f in range(F)]).astype(np.complex64)
    d_in, d_rd, d_out = ctx.alloc(F * n * 8), ctx.alloc(F * n * 8), ctx.alloc(F * A * S * C * 8)
    d_in.upload(cubes)
    got = {}
    for no_split in ("0", "1"):
        monkeypatch.setenv("MMW_NO_SPLIT_RD", no_split)
        d_rd.zero()
        _lib.check(L.mmw_range_doppler(h, d_in.ptr, d_rd.ptr, None, F, V, S, C))
        got[no_split] = d_rd.download((F, V, S, C), np.complex64)
    monkeypatch.delenv("MMW_NO_SPLIT_RD")
    for f in range(F):
        ref = O.range_doppler(cubes[f])
        for key in got:
            assert rel_err(got[key][f], ref) <= SPEC_TOL, key
    _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_out.ptr, F, V, S, C, A, 0))
    out = d_out.download((F, A, S, C), np.complex64)
    for f in (0, F - 1):
        assert rel_err(out[f], O.fft3d_windowed(cubes[f], A)) <= SPEC_TOL
    for b in (d_in, d_rd, d_out):
        b.free()


@pytest.mark.parametrize("acquire_sleep_ms", [0, 30])
def test_two_contexts_on_one_device_share_the_synchronised_chain(acquire_sleep_ms, monkeypatch):
    """Two contexts of one process on the SAME device, each driving large batches through mmw_chain3d from its own thread.
    Only one context at a time may keep the two persistent kernels of the device-synchronised schedule resident
    (sync_slot_acquire in mmw_tu_chain.hip); the other takes the event schedule for that call.  Both must finish without the
    hand-off timing out and produce the single-context result.  Second case: a sleep between a context's acquire and its
    launches (test hook) -- the other thread arrives inside that window and must still be turned away (the slot
    used to look free until the owner had recorded its events); no call may have needed the timeout re-run."""
    import threading
    if acquire_sleep_ms:
        monkeypatch.setenv("MMW_SYNC_SLOT_TEST_SLEEP_MS", str(acquire_sleep_ms))
    S, C, V, A, F = 256, 128, 12, 64, 300
    base = _lib.default_context()
    ctxs = [_lib.Context(base.device) for _ in range(2)]
    outs, errs = [None, None], []

    def work(i):
        try:
            ctx = ctxs[i]
            d_in, d_out = ctx.alloc(F * V * S * C * 8), ctx.alloc(F * A * S * C * 8)
            _lib.check(ctx.lib.mmw_synth_cubes(ctx.handle, d_in.ptr, F, V, S, C, 31337, 8, 30.0))
            for _ in range(4):
                _lib.check(ctx.lib.mmw_chain3d(ctx.handle, d_in.ptr, None, d_out.ptr, F, V, S, C, A, 0))
            ctx.sync()
            outs[i] = d_out.download((F, A, S, C), np.complex64)[[0, F // 2, F - 1]]
            d_in.free()
            d_out.free()
        except Exception as exc:        # noqa: BLE001 - reported below, in the main thread
            errs.append(exc)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    assert cross_schedule_dev(outs[0], outs[1]) <= CROSS_SCHEDULE_TOL
    for c in ctxs:
        p = (_lib.C.c_int * 8)()
        _lib.check(c.lib.mmw_diag_chain_plan(c.handle, F, V, S, C, A, 0, p))
        assert p[5] == 0, "a chain call timed out and was re-run: two contexts held the synchronised schedule at once"
    d_in = base.alloc(V * S * C * 8)
    _lib.check(base.lib.mmw_synth_cubes(base.handle, d_in.ptr, 1, V, S, C, 31337, 8, 30.0))
    cube0 = d_in.download((V, S, C), np.complex64)
    assert rel_err(outs[0][0], O.fft3d_windowed(cube0, A)) <= SPEC_TOL
    d_in.free()
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("nrx,ntx,S,C,F", [(4, 3, 63, 100, 500), (4, 3, 254, 50, 120), (4, 2, 64, 40, 700), (4, 3, 63, 127, 150)])
def test_raw_cube_device_synchronised_chain_on_shipped_shapes(monkeypatch, nrx, ntx, S, C, F):
    """mmw_chain3d_raw through the device-synchronised schedule with the raw-cube producer of the compile-time kernels
    (k_rd_mixed_ct MODE 3: every ntx-th chirp of a raw row, rx-major hand-out order): bit-identical to
    mmw_virtual_array_reformat + mmw_chain3d on the same schedule, and equal to the serial raw chain to float32 rounding."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    V, A = nrx * ntx, 64
    rng = np.random.default_rng(S * C + F)
    raw = (rng.integers(-512, 512, (F, nrx, S, ntx * C)) + 1j * rng.integers(-512, 512, (F, nrx, S, ntx * C))).astype(np.complex64)
    d_raw, d_virt = ctx.alloc(raw.nbytes), ctx.alloc(raw.nbytes)
    d_a, d_b = ctx.alloc(F * A * S * C * 8), ctx.alloc(F * A * S * C * 8)
    d_raw.upload(raw)
    _lib.check(L.mmw_virtual_array_reformat(h, d_raw.ptr, d_virt.ptr, F, nrx, ntx, S, C))

    def plan(mode):
        monkeypatch.setenv("MMW_CHAIN_PIPELINE", "0" if mode == "serial" else "1")
        monkeypatch.setenv("MMW_CHAIN_MODE", "sync")

    plan("sync")
    # planes with a 127-point level: the virtual-array producer takes the bfloat16 x 3 form of that level by default, the
    # raw-cube producer keeps the float32 MFMAs (registers) -- bit-identical with both on the float32 form, float32
    # rounding apart with the defaults
    big_prime = 127 in (S, C) or 254 in (S, C)
    try:
        if big_prime:
            ctx.set_option("MMW_BIGPRIME_BF16", 0)
        _lib.check(L.mmw_chain3d(h, d_virt.ptr, None, d_a.ptr, F, V, S, C, A, 0))
        _lib.check(L.mmw_chain3d_raw(h, d_raw.ptr, None, d_b.ptr, F, nrx, ntx, S, C, A, 0))
        a, b = d_a.download((F, A, S, C), np.complex64), d_b.download((F, A, S, C), np.complex64)
        np.testing.assert_array_equal(a, b)
    finally:
        ctx.set_option("MMW_BIGPRIME_BF16", None)
    if big_prime:
        _lib.check(L.mmw_chain3d(h, d_virt.ptr, None, d_a.ptr, F, V, S, C, A, 0))
        a = d_a.download((F, A, S, C), np.complex64)
        assert cross_schedule_dev(b, a) <= CROSS_SCHEDULE_TOL
    plan("serial")
    d_b.zero()
    _lib.check(L.mmw_chain3d_raw(h, d_raw.ptr, None, d_b.ptr, F, nrx, ntx, S, C, A, 0))
    assert cross_schedule_dev(d_b.download((F, A, S, C), np.complex64), a) <= CROSS_SCHEDULE_TOL
    virt0 = d_virt.download((V, S, C), np.complex64)
    assert rel_err(a[0], O.fft3d_windowed(virt0, A)) <= SPEC_TOL
    for buf in (d_raw, d_virt, d_a, d_b):
        buf.free()


def test_download_results_come_from_a_pinned_pool_and_stay_caller_owned():
    """Downloads of 1 MiB and more on the default context land in pooled pinned blocks (``Context.result_array``): every result
    is a fresh, writable array of its own while it is alive (the reference hands out fresh ndarrays), and a dropped result's
    block is what the next download of that size gets."""
    import gc
    ctx = _lib.default_context()
    if ctx._result_pool is None:
        pytest.skip("MMW_PINNED_RESULTS=0")
    n = 3 << 20
    d = ctx.alloc(n)
    src = np.arange(n // 4, dtype=np.float32)
    d.upload(src)
    a = d.download((n // 4,), np.float32)
    b = d.download((n // 4,), np.float32)
    addr_a, addr_b = a.__array_interface__["data"][0], b.__array_interface__["data"][0]
    assert addr_a != addr_b and a.flags.writeable and b.flags.writeable
    np.testing.assert_array_equal(a, src)
    a[:] = -1.0                                      # the caller owns it: b and the device copy are untouched
    np.testing.assert_array_equal(b, src)
    view = a[100:200]
    del a
    gc.collect()
    c = d.download((n // 4,), np.float32)            # a view still holds the first block: a third one
    assert c.__array_interface__["data"][0] not in (addr_a, addr_b) and float(view[0]) == -1.0
    del view, c
    gc.collect()
    e = d.download((n // 4,), np.float32)            # now a released block comes back
    assert e.__array_interface__["data"][0] != addr_b
    np.testing.assert_array_equal(e, src)
    small = d.download((16,), np.float32)            # small results: plain NumPy memory
    assert small.base is None
    # a block larger than what the pool may still take frees idle blocks of other sizes instead of ending the pooling
    del e, b
    gc.collect()
    held = ctx._result_bytes
    assert held >= 3 * (4 << 20)                     # the three 4 MiB blocks of above, idle now
    big_n = (_lib.RESULT_POOL_CAP - held + (1 << 20)) // 4
    d_big = ctx.alloc(big_n * 4)
    big = d_big.download((big_n,), np.float32)
    assert big.base is not None and ctx._result_bytes <= _lib.RESULT_POOL_CAP
    del big
    gc.collect()
    d_big.free()
    d.free()


def test_chirpz_plan_cache_eviction():
    """The context keeps at most 8 chirp-z plans (mmw_czt.h); a ninth frequency list drops the oldest.  Twelve lists in a
    row, then the first again: every result against the float64 sum."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    V, S, C, m = 4, 64, 8, 40
    cube = synth.synth_cube(77, (V, S, C)).astype(np.complex64)
    d_in, d_out = ctx.alloc(cube.nbytes), ctx.alloc(m * 4)
    d_in.upload(cube[None])
    x = cube[:, :, 2].astype(complex) * np.hanning(S)[None, :]
    params = [(0.01 + 0.013 * i, 0.0009 + 0.0001 * i) for i in range(12)] + [(0.01, 0.0009)]
    for f0, df in params:
        _lib.check(L.mmw_range_zoom(h, d_in.ptr, d_out.ptr, 1, V, S, C, 2, m, f0, df))
        got = d_out.download((m,), np.float32)
        Z = np.exp(-2j * np.pi * np.outer(f0 + df * np.arange(m), np.arange(S)))
        assert rel_err(got, np.mean(np.abs(x @ Z.T), axis=0)) <= SPEC_TOL, (f0, df)
    d_in.free()
    d_out.free()


@pytest.mark.parametrize("S,C,F", [(63, 100, 400), (90, 100, 300), (63, 127, 200)])
def test_device_synchronised_chain_magnitude_output_on_misaligned_rows(monkeypatch, S, C, F):
    """MMW_ANGLE_MAGNITUDE through the synchronised chain on planes whose float32 rows are not 64-B aligned (row-window
    consumer with 16-cell units; 63 x 127 is odd and takes the event schedule with the generic |.| kernel): against the
    serial schedule and the oracle."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    V, A = 12, 64
    d_in, d_out = ctx.alloc(F * V * S * C * 8), ctx.alloc(F * A * S * C * 4)
    _lib.check(L.mmw_synth_cubes(h, d_in.ptr, F, V, S, C, 4711, 6, 30.0))
    outs = {}
    for mode in ("serial", "sync"):
        monkeypatch.setenv("MMW_CHAIN_PIPELINE", "0" if mode == "serial" else "1")
        monkeypatch.setenv("MMW_CHAIN_MODE", "sync")
        d_out.zero()
        _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_out.ptr, F, V, S, C, A, _lib.ANGLE_MAGNITUDE))
        outs[mode] = d_out.download((F, A, S, C), np.float32)
    assert cross_schedule_dev(outs["sync"], outs["serial"]) <= CROSS_SCHEDULE_TOL
    cube = d_in.download((V, S, C), np.complex64, byte_offset=(F - 1) * V * S * C * 8)
    assert rel_err(outs["sync"][F - 1], np.abs(O.fft3d_windowed(cube, A))) <= SPEC_TOL
    d_in.free()
    d_out.free()


def _shipped_cube_shapes():
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as f:
        d = json.load(f)
    return sorted({(e["expect"]["num_rx"] * e["expect"]["num_tx"], e["expect"]["num_samples"], e["expect"]["loops"])
                   for e in d.values()})


@pytest.mark.parametrize("V,S,C", _shipped_cube_shapes())
def test_every_shipped_cfg_shape_through_the_synchronised_chain(monkeypatch, V, S, C):
    """Every cube shape (virtual antennas x samples x loops) of the cfg files the reference ships, 160 frames through
    mmw_chain3d on the serial and on the device-synchronised schedule: the plan must say 'synchronised' (each of them has a
    single-pass range-Doppler producer and an angle consumer), the schedules agree to float32 rounding and the first and
    last frame match the oracle."""
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    A, F = 64, 160
    d_in, d_out = ctx.alloc(F * V * S * C * 8), ctx.alloc(F * A * S * C * 8)
    _lib.check(L.mmw_synth_cubes(h, d_in.ptr, F, V, S, C, 9000 + S + C, 6, 30.0))
    outs = {}
    for mode in ("serial", "sync"):
        monkeypatch.setenv("MMW_CHAIN_PIPELINE", "0" if mode == "serial" else "1")
        monkeypatch.setenv("MMW_CHAIN_MODE", "sync")
        plan = (_lib.C.c_int * 8)()
        _lib.check(L.mmw_diag_chain_plan(h, F, V, S, C, A, 0, plan))
        assert bool(plan[6]) == (mode == "sync"), (mode, list(plan))
        d_out.zero()
        _lib.check(L.mmw_chain3d(h, d_in.ptr, None, d_out.ptr, F, V, S, C, A, 0))
        outs[mode] = d_out.download((F, A, S, C), np.complex64)
    assert cross_schedule_dev(outs["sync"], outs["serial"]) <= CROSS_SCHEDULE_TOL
    for f in (0, F - 1):
        cube = d_in.download((V, S, C), np.complex64, byte_offset=f * V * S * C * 8)
        assert rel_err(outs["sync"][f], O.fft3d_windowed(cube, A)) <= SPEC_TOL
    d_in.free()
    d_out.free()


def test_int16_iq_ingest_matches_the_complex64_raw_path():
    """mmw_virtual_array_reformat_i16 / FramePipeline.load_raw_i16 (int16 I/Q pairs, NO UPSTREAM ORACLE for the sample layout:
    defined as the raw cube of load_raw with int16 pairs) == load_raw on the same samples as complex64, bit for bit, and the
    chain on top of it matches the oracle."""
    from mmwave_radar_processing_amd.batch import FramePipeline
    F, nrx, ntx, S, C = 3, 4, 3, 63, 100
    cm = make_cm(synth.synth_cfg_text(num_samples=S, num_loops=C))
    rng = np.random.default_rng(16)
    iq = rng.integers(-2048, 2048, (F, nrx, S, ntx * C, 2)).astype(np.int16)
    raw = (iq[..., 0].astype(np.float32) + 1j * iq[..., 1].astype(np.float32)).astype(np.complex64)
    a = FramePipeline(cm, max_frames=F, shape=(nrx * ntx, S, C))
    b = FramePipeline(cm, max_frames=F, shape=(nrx * ntx, S, C))
    a.load_raw(raw, ntx)
    b.load_raw_i16(iq, ntx)
    np.testing.assert_array_equal(a.cubes(0, F), b.cubes(0, F))
    b.chain3d()
    assert rel_err(b.fetch_chain3d(F - 1), O.fft3d_windowed(a.cubes(F - 1, F)[0])) <= SPEC_TOL
    with pytest.raises(ValueError):
        b.load_raw_i16(iq[..., 0], ntx)


def _detect_points_raw(ctx, d_in, F, shape, cfar, cap, az, el, A=64):
    """mmw_detect_points on resident cubes -> (counts, dets, az_idx, el_idx, stats)."""
    V, S, C = shape
    (tr, td), (gr, gd) = cfar.num_train, cfar.num_guard
    d_rd, d_l1 = ctx.alloc(F * V * S * C * 8), ctx.alloc(F * V * 4)
    d_dets, d_cnt = ctx.alloc(F * cap * 8), ctx.alloc(F * 4)
    d_az, d_el = ctx.alloc(F * cap * 4), ctx.alloc(F * cap * 4)
    a_az, n_az = _lib.int_array(az)
    a_el, n_el = _lib.int_array(el)
    stats = (_lib.C.c_int * 5)()
    _lib.check(ctx.lib.mmw_detect_points(ctx.handle, d_in.ptr, d_rd.ptr, d_l1.ptr, None, d_dets.ptr, d_cnt.ptr, d_az.ptr, d_el.ptr,
                                         F, V, S, C, cfar.kind, int(tr), int(td), int(gr), int(gd), float(cfar._scale()),
                                         int(cfar._k_rank()), cap, a_az, n_az, 1, a_el, n_el, 0, A, stats))
    out = (d_cnt.download((F,), np.int32), d_dets.download((F, cap, 2), np.int32), d_az.download((F, cap), np.int32),
           d_el.download((F, cap), np.int32), list(stats))
    for b in (d_rd, d_l1, d_dets, d_cnt, d_az, d_el):
        b.free()
    return out


def _detect_float64_raw(ctx, d_in, F, shape, cfar, cap, az, el, A=64):
    """The float64 path (mmw_detect_batch + mmw_angle_argmax_exact) on the same cubes."""
    V, S, C = shape
    (tr, td), (gr, gd) = cfar.num_train, cfar.num_guard
    n = S * C
    d_rd, d_l1, d_mag, d_mask = ctx.alloc(F * V * n * 8), ctx.alloc(F * V * 4), ctx.alloc(F * n * 8), ctx.alloc(F * n)
    d_dets, d_cnt = ctx.alloc(F * cap * 8), ctx.alloc(F * 4)
    d_az, d_el = ctx.alloc(F * cap * 4), ctx.alloc(F * cap * 4)
    _lib.check(ctx.lib.mmw_detect_batch(ctx.handle, d_in.ptr, d_rd.ptr, d_mag.ptr, d_mask.ptr, d_dets.ptr, d_cnt.ptr, d_l1.ptr, F, V,
                                        S, C, cfar.kind, int(tr), int(td), int(gr), int(gd), float(cfar._scale()),
                                        int(cfar._k_rank()), cap))
    for ant, d_idx, shift in ((az, d_az, 1), (el, d_el, 0)):
        arr, n_ant = _lib.int_array(ant)
        _lib.check(ctx.lib.mmw_angle_argmax_exact(ctx.handle, d_in.ptr, d_l1.ptr, d_rd.ptr, d_dets.ptr, d_cnt.ptr, d_idx.ptr, F, V, S,
                                                  C, cap, arr, n_ant, A, shift, None))
    out = (d_cnt.download((F,), np.int32), d_dets.download((F, cap, 2), np.int32), d_az.download((F, cap), np.int32),
           d_el.download((F, cap), np.int32))
    for b in (d_rd, d_l1, d_mag, d_mask, d_dets, d_cnt, d_az, d_el):
        b.free()
    return out


def _same_points(got, ref):
    cnt, dets, az, el = got[:4]
    cnt_r, dets_r, az_r, el_r = ref[:4]
    np.testing.assert_array_equal(cnt, cnt_r)
    for f in range(cnt.shape[0]):
        k = int(cnt[f])
        np.testing.assert_array_equal(dets[f, :k], dets_r[f, :k])
        np.testing.assert_array_equal(az[f, :k], az_r[f, :k])
        np.testing.assert_array_equal(el[f, :k], el_r[f, :k])


@pytest.mark.parametrize("shape,frames", [((12, 256, 128), 160), ((12, 63, 100), 400), ((8, 64, 32), 300), ((12, 254, 50), 64),
                                          ((12, 512, 128), 24), ((4, 127, 32), 96), ((8, 63, 127), 48)])
def test_detect_points_screening_equals_the_float64_path(shape, frames, monkeypatch):
    """mmw_detect_points (float32 screening with the worst-case error band + float64 decision of the undecided cells)
    against mmw_detect_batch + mmw_angle_argmax_exact on the same resident cubes: counts, detections (values and order)
    and both argmax index arrays identical; then with the band widened 50x (many cells through k_cfar_cell_exact)."""
    V, S, C = shape
    ctx = _lib.default_context()
    cfar = CaCFAR2D((4, 4), (2, 2), 1e-5)
    az, el = list(range(min(8, V))), list(range(max(0, V - 4), V))
    d_in = ctx.alloc(frames * V * S * C * 8)
    _lib.check(ctx.lib.mmw_synth_cubes(ctx.handle, d_in.ptr, frames, V, S, C, 424242, 8, 30.0))
    assert ctx.lib.mmw_detect_points_supported(S, C, cfar.kind, 4, 4, 2, 2, len(az), len(el), 64) == 1
    ref = _detect_float64_raw(ctx, d_in, frames, shape, cfar, 1024, az, el)
    got = _detect_points_raw(ctx, d_in, frames, shape, cfar, 1024, az, el)
    _same_points(got, ref)
    print(f"{shape}: {frames} frames, {int(ref[0].sum())} detections; screening left {got[4][1]} cells in {got[4][0]} frames "
          f"undecided, {got[4][2]} frames handed back, {got[4][3]} + {got[4][4]} argmax evaluations refined")
    assert got[4][2] == 0 and ref[0].sum() > frames
    # ... and not only each other: the oracle (float64 NumPy restatement of the reference) on the first frames of every shape
    for f in range(3):
        cube = d_in.download((V, S, C), np.complex64, f * V * S * C * 8)
        raw, _, dets_ref, _, _ = O.rd_detect_2d(cube, (4, 4), (2, 2), 1e-5)
        k = int(got[0][f])
        np.testing.assert_array_equal(got[1][f, :k], dets_ref)
        if k:
            r, v = dets_ref[:, 0].astype(int), dets_ref[:, 1].astype(int)
            np.testing.assert_array_equal(got[2][f, :k], O.angle_argmax(raw, r, v, az, 64, True)[0])
            np.testing.assert_array_equal(got[3][f, :k], O.angle_argmax(raw, r, v, el, 64, False)[0])
    # the angle estimates come from the tail's record kernels by default (late argmax); the in-kernel form gives the same
    try:
        ctx.set_option("MMW_DETECT_LATE_ARGMAX", 0)
        inside = _detect_points_raw(ctx, d_in, frames, shape, cfar, 1024, az, el)
    finally:
        ctx.set_option("MMW_DETECT_LATE_ARGMAX", None)
    _same_points(inside, ref)
    monkeypatch.setenv("MMW_DETECT_BAND_MULT", "50")
    wide = _detect_points_raw(ctx, d_in, frames, shape, cfar, 1024, az, el)
    handed_back = wide[0] < 0
    assert wide[4][1] > got[4][1] and handed_back.sum() == wide[4][2]
    keep = ~handed_back
    _same_points(tuple(x[keep] for x in wide[:4]), tuple(x[keep] for x in ref))
    print(f"  band x50: {wide[4][1]} undecided cells in {wide[4][0]} frames, {wide[4][2]} frames handed back")
    d_in.free()


@pytest.mark.parametrize("shape,frames,az,el", [((16, 64, 32), 200, list(range(12)), list(range(7, 16))),
                                                ((12, 256, 128), 48, list(range(12)), [11, 3, 7, 0, 5, 9, 1, 8, 2, 10]),
                                                ((16, 63, 100), 120, list(range(16)), [15, 14, 13])])
def test_detect_points_with_lists_of_nine_to_sixteen_antennas(shape, frames, az, el):
    """Antenna lists of 9 to 16 entries (point_cloud_generator.py:143-214 accepts any list) through the fused stage: with 64
    angle bins the angle estimates are the tail's lane-per-detection launches (16 / N register FFTs of N = 16 points), with
    the same worst-case bound and pairwise test; identical to the float64 path and to the oracle.  The band is widened so
    that speculative slots and flagged evaluations occur.  Without the late argmax such lists have no fused kernel."""
    ctx = _lib.default_context()
    V, S, C = shape
    cfar = CaCFAR2D((4, 4), (2, 2), 1e-4)
    d_in = ctx.alloc(frames * V * S * C * 8)
    _lib.check(ctx.lib.mmw_synth_cubes(ctx.handle, d_in.ptr, frames, V, S, C, 171717, 8, 30.0))
    assert ctx.lib.mmw_detect_points_supported(S, C, cfar.kind, 4, 4, 2, 2, len(az), len(el), 64) == 1
    assert ctx.lib.mmw_detect_points_supported(S, C, cfar.kind, 4, 4, 2, 2, len(az), len(el), 128) == 0
    ref = _detect_float64_raw(ctx, d_in, frames, shape, cfar, 512, az, el)
    try:
        ctx.set_option("MMW_DETECT_BAND_MULT", 20)
        got = _detect_points_raw(ctx, d_in, frames, shape, cfar, 512, az, el)
        ctx.set_option("MMW_DETECT_LATE_ARGMAX", 0)
        with pytest.raises(_lib.MmwGpuError):
            _detect_points_raw(ctx, d_in, frames, shape, cfar, 512, az, el)
    finally:
        ctx.set_option("MMW_DETECT_BAND_MULT", None)
        ctx.set_option("MMW_DETECT_LATE_ARGMAX", None)
    keep = got[0] >= 0
    assert keep.sum() >= frames // 2 and ref[0].sum() > frames
    _same_points(tuple(x[keep] for x in got[:4]), tuple(x[keep] for x in ref))
    print(f"{shape}, lists of {len(az)} / {len(el)} antennas: {int(ref[0].sum())} detections in {frames} frames, {got[4][1]} cells decided in "
          f"float64, {got[4][3]} + {got[4][4]} evaluations refined, {int((~keep).sum())} frames handed back")
    for f in np.nonzero(keep)[0][:3]:
        cube = d_in.download((V, S, C), np.complex64, int(f) * V * S * C * 8)
        raw, _, dets_ref, _, _ = O.rd_detect_2d(cube, (4, 4), (2, 2), 1e-4)
        k = int(got[0][f])
        np.testing.assert_array_equal(got[1][f, :k], dets_ref)
        if k:
            r, v = dets_ref[:, 0].astype(int), dets_ref[:, 1].astype(int)
            np.testing.assert_array_equal(got[2][f, :k], O.angle_argmax(raw, r, v, az, 64, True)[0])
            np.testing.assert_array_equal(got[3][f, :k], O.angle_argmax(raw, r, v, el, 64, False)[0])
    d_in.free()


def test_detect_points_edge_cases_and_pipeline_fallback(monkeypatch):
    """Zero cubes, a window larger than the plane, a detection capacity that overflows, non-finite samples in antenna 0
    (count -1 -> FramePipeline runs the frame through the float64 path) and a band so wide that every frame is handed back."""
    from mmwave_radar_processing_amd.batch import FramePipeline
    ctx = _lib.default_context()
    shape = (12, 64, 32)
    V, S, C = shape
    cfar = CaCFAR2D((4, 4), (2, 2), 1e-3)
    az, el = list(range(8)), [8, 9, 10, 11]
    cubes = np.stack([synth.synth_cube(7100 + f, shape) for f in range(6)])
    cubes[1] = 0
    cubes[3, 0, 5, 7] = np.inf
    cubes[4, 0, 9, 1] = np.nan
    d_in = ctx.alloc(cubes.nbytes)
    d_in.upload(cubes)
    got = _detect_points_raw(ctx, d_in, 6, shape, cfar, 256, az, el)
    assert got[0][1] == 0 and got[0][3] == -1 and got[0][4] == -1 and got[4][2] == 2
    ref = _detect_float64_raw(ctx, d_in, 6, shape, cfar, 256, az, el)
    keep = got[0] >= 0
    _same_points(tuple(x[keep] for x in got[:4]), tuple(x[keep] for x in ref))
    # capacity overflow: exact counts, the first cap detections in order
    small = _detect_points_raw(ctx, d_in, 6, shape, cfar, 3, az, el)
    np.testing.assert_array_equal(small[0][keep], ref[0][keep])
    for f in np.nonzero(keep)[0]:
        k = min(3, int(ref[0][f]))
        np.testing.assert_array_equal(small[1][f, :k], ref[1][f, :k])
        np.testing.assert_array_equal(small[2][f, :k], ref[2][f, :k])
    # window larger than the plane: no detections, no error (ca_cfar.py:99-102)
    big = CaCFAR2D((40, 4), (2, 2), 1e-3)
    assert np.all(_detect_points_raw(ctx, d_in, 6, shape, big, 16, az, el)[0][[0, 1, 2, 5]] == 0)
    d_in.free()
    # the pipeline hands frames the screening cannot decide to the float64 path
    cm = make_cm(synth.synth_cfg_text(num_samples=S, num_loops=C))
    sc = O.cfg_scalars(synth.synth_cfg_text(num_samples=S, num_loops=C))
    pipe = FramePipeline(cm, max_frames=6, shape=shape, cfar=cfar, az_antenna_idxs=az, el_antenna_idxs=el)
    finite = cubes.copy()
    finite[3, 0, 5, 7] = 0
    finite[4, 0, 9, 1] = 0
    monkeypatch.setenv("MMW_DETECT_BAND_MULT", "100000000")
    pipe.load(finite)
    pcs = pipe.point_clouds()
    # (the zero frame has a zero band: it is decided; a frame with more undecided cells than it can carry is handed back)
    assert pipe.screen_stats[2] >= 1 and pipe.screen_stats[1] >= 32
    for f in range(6):
        pc_ref, dets_ref, az_i, el_i = O.point_cloud(finite[f], sc, az, el, num_train=(4, 4), num_guard=(2, 2), pfa=1e-3)
        np.testing.assert_array_equal(pipe.dets[f], dets_ref)
        if dets_ref.shape[0]:
            np.testing.assert_array_equal(pipe.az_idx[f], az_i)
            np.testing.assert_array_equal(pipe.el_idx[f], el_i)
            np.testing.assert_allclose(pcs[f], pc_ref, rtol=0, atol=1e-9 * sc["range_max_m"])


@pytest.mark.parametrize("shape,F", [((12, 256, 128), 96), ((12, 63, 100), 300), ((8, 254, 50), 200)])
def test_detect_points_deferred_tail_back_to_back(shape, F):
    """mmw_detect_points does not join its tail (exact cells, list insertion, float64 refinement) at the end of a call: the next
    call's range-Doppler launch runs beside it, every other entry point joins it first.  Back-to-back calls -- same buffers
    again, then other inputs into other buffers -- with the band widened (so that there ARE undecided cells and flagged
    evaluations) leave exactly what calls that join their own tail leave (MMW_DETECT_DEFER_TAIL=0 / the statistics request).
    256 x 128: the ticketed range-Doppler pair behind the tail; the shipped shapes: their compile-time mixed-radix kernels
    (one workgroup per plane at 63 x 100, the persistent form at 254 x 50)."""
    cap = 512
    V, S, C = shape
    ctx = _lib.Context(0)
    ctx.set_option("MMW_DETECT_BAND_MULT", 20)
    cfar = CaCFAR2D((4, 4), (2, 2), 1e-5)
    az, el = list(range(min(8, V))), list(range(max(0, V - 4), V))
    a_az, n_az = _lib.int_array(az)
    a_el, n_el = _lib.int_array(el)
    d_a, d_b = ctx.alloc(F * V * S * C * 8), ctx.alloc(F * V * S * C * 8)
    _lib.check(ctx.lib.mmw_synth_cubes(ctx.handle, d_a.ptr, F, V, S, C, 515151, 8, 30.0))
    _lib.check(ctx.lib.mmw_synth_cubes(ctx.handle, d_b.ptr, F, V, S, C, 626262, 8, 30.0))
    ref_a = _detect_points_raw(ctx, d_a, F, shape, cfar, cap, az, el)      # (asks for the statistics: joins its own tail)
    ref_b = _detect_points_raw(ctx, d_b, F, shape, cfar, cap, az, el)
    assert ref_a[4][1] > 0 and ref_a[4][3] + ref_a[4][4] > 0, ref_a[4]      # undecided cells and flagged evaluations exist

    def buffers():
        return [ctx.alloc(n) for n in (F * V * S * C * 8, F * V * 4, F * cap * 8, F * 4, F * cap * 4, F * cap * 4)]

    def call(d_in, b):
        _lib.check(ctx.lib.mmw_detect_points(ctx.handle, d_in.ptr, b[0].ptr, b[1].ptr, None, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr,
                                             F, V, S, C, cfar.kind, 4, 4, 2, 2, float(cfar._scale()), 0, cap, a_az, n_az, 1, a_el, n_el,
                                             0, 64, None))

    def result(b):
        return (b[3].download((F,), np.int32), b[2].download((F, cap, 2), np.int32), b[4].download((F, cap), np.int32),
                b[5].download((F, cap), np.int32))

    b1, b2 = buffers(), buffers()
    for defer in (1, 0):
        ctx.set_option("MMW_DETECT_DEFER_TAIL", defer)
        for b in (b1, b2):
            for x in b[2:]:
                x.upload(np.full(x.nbytes // 4, -7, np.int32))
        call(d_a, b1)           # A into b1 ...
        call(d_a, b1)           # ... again into the same buffers (its range-Doppler launch runs beside the first call's tail)
        call(d_b, b2)           # B into other buffers, behind A's tail
        call(d_a, b1)
        got_a, got_b = result(b1), result(b2)       # (a download joins the pending tail)
        for got, ref in ((got_a, ref_a), (got_b, ref_b)):
            np.testing.assert_array_equal(got[0], ref[0])
            keep = ref[0] >= 0
            _same_points(tuple(x[keep] for x in got), tuple(x[keep] for x in ref[:4]))
    for b in b1 + b2 + [d_a, d_b]:
        b.free()
    ctx.close()


def test_detect_points_overlapped_schedule(monkeypatch):
    """The device-synchronised form of mmw_detect_points (range-Doppler producer and screening consumer side by side on
    disjoint CU sets, frames handed over through counters; the default for large batches of 256 x 128 planes, forced here
    on a small one): identical to the serial schedule and to the float64 path -- counts, detections, both argmax arrays,
    and the range-Doppler cube and L1 norms it leaves behind -- for every CU split / tail setting, with the band widened
    (cells through k_cfar_cell_exact), with frames the screening hands back, and for batches shorter than the grids."""
    shape, F = (12, 256, 128), 150
    V, S, C = shape
    ctx = _lib.Context(0)
    cfar = CaCFAR2D((4, 4), (2, 2), 1e-5)
    az, el = list(range(8)), [8, 9, 10, 11]
    d_in = ctx.alloc(F * V * S * C * 8)
    _lib.check(ctx.lib.mmw_synth_cubes(ctx.handle, d_in.ptr, F, V, S, C, 9090, 8, 30.0))
    bad = synth.synth_cube(77, shape).copy()
    bad[0, 100, 3] = np.nan                                      # frame 5: handed back by the screening
    d_in.upload(bad, 5 * V * S * C * 8)
    ctx.set_option("MMW_DETECT_OVERLAP", 0)
    serial = _detect_points_raw(ctx, d_in, F, shape, cfar, 1024, az, el)
    ref = _detect_float64_raw(ctx, d_in, F, shape, cfar, 1024, az, el)
    keep = serial[0] >= 0
    assert (~keep).sum() == 1 and not keep[5]
    _same_points(tuple(x[keep] for x in serial[:4]), tuple(x[keep] for x in ref))
    ctx.set_option("MMW_DETECT_OVERLAP", 1)
    for scr_cus, tail in ((32, 1), (32, 0), (64, 1), (128, 0)):
        ctx.set_option("MMW_DETECT_SCR_CUS", scr_cus)
        ctx.set_option("MMW_DETECT_TAIL", tail)
        got = _detect_points_raw(ctx, d_in, F, shape, cfar, 1024, az, el)
        np.testing.assert_array_equal(got[0], serial[0])
        _same_points(tuple(x[keep] for x in got[:4]), tuple(x[keep] for x in serial[:4]))
        assert got[4] == serial[4], (got[4], serial[4])
    # the cube and the norms the producer leaves behind are the serial kernel's
    d_rd, d_l1, d_rd2, d_l12 = ctx.alloc(F * V * S * C * 8), ctx.alloc(F * V * 4), ctx.alloc(F * V * S * C * 8), ctx.alloc(F * V * 4)
    d_dets, d_cnt = ctx.alloc(F * 64 * 8), ctx.alloc(F * 4)
    for ov, rd, l1 in ((1, d_rd, d_l1), (0, d_rd2, d_l12)):
        ctx.set_option("MMW_DETECT_OVERLAP", ov)
        _lib.check(ctx.lib.mmw_detect_points(ctx.handle, d_in.ptr, rd.ptr, l1.ptr, None, d_dets.ptr, d_cnt.ptr, None, None, F, V, S, C,
                                             cfar.kind, 4, 4, 2, 2, float(cfar._scale()), 0, 64, None, 0, 1, None, 0, 0, 64, None))
    for f in (0, 5, 77, F - 1):
        np.testing.assert_array_equal(d_rd.download((V, S, C), np.complex64, f * V * S * C * 8).view(np.uint32),
                                      d_rd2.download((V, S, C), np.complex64, f * V * S * C * 8).view(np.uint32))
    np.testing.assert_array_equal(d_l1.download((F, V), np.float32), d_l12.download((F, V), np.float32))
    # wide band: hundreds of cells decided in float64, some frames handed back -- same as the serial schedule's
    monkeypatch.setenv("MMW_DETECT_BAND_MULT", "50")
    ctx.set_option("MMW_DETECT_OVERLAP", 0)
    wide_s = _detect_points_raw(ctx, d_in, F, shape, cfar, 1024, az, el)
    ctx.set_option("MMW_DETECT_OVERLAP", 1)
    ctx.set_option("MMW_DETECT_SCR_CUS", 32)
    ctx.set_option("MMW_DETECT_TAIL", 1)
    wide_o = _detect_points_raw(ctx, d_in, F, shape, cfar, 1024, az, el)
    both = (wide_s[0] >= 0) & (wide_o[0] >= 0)                   # (which frames lose the race for the cell list may differ)
    assert wide_o[4][1] > 100 and both.sum() > F // 2
    _same_points(tuple(x[both] for x in wide_o[:4]), tuple(x[both] for x in ref))
    _same_points(tuple(x[both] for x in wide_s[:4]), tuple(x[both] for x in ref))
    monkeypatch.delenv("MMW_DETECT_BAND_MULT")
    # batches shorter than either grid
    for n in (1, 3, 40):
        got = _detect_points_raw(ctx, d_in, n, shape, cfar, 1024, az, el)
        np.testing.assert_array_equal(got[0], serial[0][:n])
        k = got[0] >= 0
        _same_points(tuple(x[k] for x in got[:4]), tuple(x[:n][k] for x in serial[:4]))
    print(f"overlapped detection schedule: {int(serial[0][keep].sum())} detections in {F} frames identical across schedules")
    ctx.close()


def test_detect_handoff_timeout_hands_the_frames_back():
    """The overlapped detection schedule with its producer withheld (test switch): the consumer's bounded wait gives up,
    every frame gets count -1 (the status of a frame the screening cannot decide), the call returns normally, and
    FramePipeline runs those frames through the float64 path -- results equal the oracle's; the next call is fine."""
    from mmwave_radar_processing_amd.batch import FramePipeline
    shape, F = (12, 256, 128), 24
    V, S, C = shape
    ctx = _lib.Context(0)
    cfar = CaCFAR2D((4, 4), (2, 2), 1e-5)
    az, el = list(range(8)), [8, 9, 10, 11]
    cubes = np.stack([synth.synth_cube(4400 + f, shape) for f in range(F)])
    d_in = ctx.alloc(cubes.nbytes)
    d_in.upload(cubes)
    ctx.set_option("MMW_DETECT_OVERLAP", 1)
    ctx.set_option("MMW_CHAIN_TIMEOUT_MS", 20)
    ctx.set_option("MMW_DETECT_DIAG_SKIP_RD", 1)
    import time
    t0 = time.perf_counter()
    got = _detect_points_raw(ctx, d_in, F, shape, cfar, 1024, az, el)
    dt = time.perf_counter() - t0
    assert np.all(got[0] == -1) and got[4][2] == F and dt < 2.0
    ctx.set_option("MMW_DETECT_DIAG_SKIP_RD", None)
    ok = _detect_points_raw(ctx, d_in, F, shape, cfar, 1024, az, el)
    assert np.all(ok[0] >= 0) and ok[4][2] == 0
    sc = O.cfg_scalars(synth.SYNTH_CFG_256x128x12)
    for f in (0, F - 1):
        _, dets_ref, az_i, el_i = O.point_cloud(cubes[f], sc, az, el)
        k = int(ok[0][f])
        np.testing.assert_array_equal(ok[1][f, :k], dets_ref)
        np.testing.assert_array_equal(ok[2][f, :k], az_i)
        np.testing.assert_array_equal(ok[3][f, :k], el_i)
    # the pipeline: frames handed back by the timed-out hand-off take the float64 path
    cm = make_cm(synth.SYNTH_CFG_256x128x12)
    pipe = FramePipeline(cm, max_frames=F, shape=shape, cfar=cfar, az_antenna_idxs=az, el_antenna_idxs=el, ctx=ctx)
    pipe.load(cubes)
    ctx.set_option("MMW_DETECT_DIAG_SKIP_RD", 1)
    pcs = pipe.point_clouds()
    ctx.set_option("MMW_DETECT_DIAG_SKIP_RD", None)
    assert pipe.screen_stats[2] == F
    for f in (0, 7, F - 1):
        pc_ref, dets_ref, az_i, el_i = O.point_cloud(cubes[f], sc, az, el)
        np.testing.assert_array_equal(pipe.dets[f], dets_ref)
        np.testing.assert_array_equal(pipe.az_idx[f], az_i)
        np.testing.assert_array_equal(pipe.el_idx[f], el_i)
        np.testing.assert_allclose(pcs[f], pc_ref, rtol=0, atol=1e-9 * sc["range_max_m"])
    print(f"detection hand-off timeout: {F} frames handed back in {dt * 1e3:.0f} ms and decided by the float64 path")
    ctx.close()


def test_chain_handoff_timeout_is_detected_and_rerun(monkeypatch):
    """The device-synchronised chain with its producer withheld (diagnostic hook): the consumer's bounded spin gives up,
    the next host-synchronising entry point notices, resets the hand-off state and re-runs the call on the event
    schedule -- the downloaded cube is the serial schedule's; with MMW_CHAIN_NO_RERUN=1 the download raises instead; the
    context keeps working either way (a timed-out run used to return an incomplete cube with status 0)."""
    import time
    ctx = _lib.Context(0)
    F, V, S, C, A = 96, 12, 256, 128, 64
    d_in, d_out = ctx.alloc(F * V * S * C * 8), ctx.alloc(F * A * S * C * 8)
    _lib.check(ctx.lib.mmw_synth_cubes(ctx.handle, d_in.ptr, F, V, S, C, 5150, 8, 30.0))

    def chain():
        _lib.check(ctx.lib.mmw_chain3d(ctx.handle, d_in.ptr, None, d_out.ptr, F, V, S, C, A, 0))

    def plan():
        p = (_lib.C.c_int * 8)()
        _lib.check(ctx.lib.mmw_diag_chain_plan(ctx.handle, F, V, S, C, A, 0, p))
        return list(p)

    picks = (0, 47, 95)
    fetch = lambda: [d_out.download((A, S, C), np.complex64, f * A * S * C * 8) for f in picks]
    monkeypatch.setenv("MMW_CHAIN_PIPELINE", "0")
    chain()
    ref = fetch()
    monkeypatch.setenv("MMW_CHAIN_PIPELINE", "1")
    monkeypatch.setenv("MMW_CHAIN_TIMEOUT_MS", "20")
    assert plan()[6] == 1 and plan()[5] == 0                    # device-synchronised form, nothing re-run so far
    # 1. producer withheld: the call itself returns at once, the sync settles it
    d_out.zero()
    monkeypatch.setenv("MMW_CHAIN_DIAG_SKIP_RD", "1")
    chain()
    monkeypatch.delenv("MMW_CHAIN_DIAG_SKIP_RD")
    t0 = time.perf_counter()
    ctx.sync()
    dt = time.perf_counter() - t0
    assert plan()[5] == 1, "the timed-out call was not re-run"
    got = fetch()
    for a, b in zip(got, ref):
        assert rel_err(a, b) <= 1e-6
    print(f"hand-off timeout detected and call re-run on the event schedule in {dt * 1e3:.0f} ms")
    assert dt < 2.0
    # 2. the very next device-synchronised call on the same context is fine (fresh ring layout)
    d_out.zero()
    chain()
    got = fetch()
    assert plan()[5] == 1
    for a, b in zip(got, ref):
        assert rel_err(a, b) <= 1e-6
    # 3. no automatic re-run: the fetch path reports the timeout (it used to hand back an incomplete cube with status 0)
    monkeypatch.setenv("MMW_CHAIN_NO_RERUN", "1")
    monkeypatch.setenv("MMW_CHAIN_DIAG_SKIP_RD", "1")
    d_out.zero()
    chain()
    monkeypatch.delenv("MMW_CHAIN_DIAG_SKIP_RD")
    with pytest.raises(_lib.MmwGpuError, match="timed out"):
        d_out.download((A, S, C), np.complex64, 0)
    monkeypatch.delenv("MMW_CHAIN_NO_RERUN")
    chain()
    got = fetch()
    for a, b in zip(got, ref):
        assert rel_err(a, b) <= 1e-6
    d_in.free()
    d_out.free()
    ctx.close()


# ---- detectors the reference's shipped YAMLs use, against fixtures generated by the reference itself
#      (tests/golden/make_golden.py::gen_detectors_rd -> detectors_rd.npz; oracle == fixtures in test_oracle_golden.py)
from test_oracle_golden import GOSO_SEQ, GROUND, YAML_OS2D, YAML_SEQ, _rd_cases      # noqa: E402


def _cm_for(tag):
    if tag == "np2":
        with open(os.path.join(GOLDEN, "cfg_scalars.json")) as fh:
            return make_cm("\n".join(json.load(fh)["6843_RadVel_ods_20Hz.cfg"]["lines"]))
    return make_cm(synth.SYNTH_CFG_256x128x12)


def test_sequential_and_os2d_detectors_match_reference_fixtures():
    g = np.load(os.path.join(GOLDEN, "detectors_rd.npz"))
    for tag, _, cube in _rd_cases():
        cm = _cm_for(tag)
        for key, (rk, rp, vk, vp) in (("seq_yaml", YAML_SEQ), ("seq_goso", GOSO_SEQ)):
            det = RangeDopplerDetectorSequential(cm, rng_cfar_type=rk, rng_cfar_params=rp, vel_cfar_type=vk, vel_cfar_params=vp)
            got = det.process(cube)
            np.testing.assert_array_equal(got, g[f"{tag}_{key}"])
            assert got.dtype == g[f"{tag}_{key}"].dtype
        det2 = RangeDopplerDetector2D(cm, cfar_type="os_cfar_2d",
                                      cfar_params={"num_train": [5, 5], "num_guard": [3, 2], "rho": 0.7, "alpha": 2})
        np.testing.assert_array_equal(det2.process(cube), g[f"{tag}_os2d_yaml"])
    # the batch pipeline with the same OS detector (mask-by-counting kernel) on the four headline frames
    from mmwave_radar_processing_amd.batch import FramePipeline
    cm = _cm_for("s0")
    pipe = FramePipeline(cm, max_frames=4, shape=(12, 256, 128), cfar=OsCFAR2D([5, 5], [3, 2], rho=0.7, alpha=2))
    pipe.load(np.stack([synth.synth_cube(s) for s in range(4)]))
    for s, d in enumerate(pipe.detect()):
        np.testing.assert_array_equal(d, g[f"s{s}_os2d_yaml"])


def test_detectors_on_more_non_power_of_two_shapes_match_reference_fixtures():
    """PointCloudGenerator (CA-CFAR 2-D: the fused stage on the compile-time mixed-radix RD kernels), RangeDopplerDetector2D with
    the GUI's OS-CFAR and the YAML sequential detector on four more shipped cfg shapes, against fixtures generated by the
    imported reference (tests/golden/detectors_np2.npz): detections identical, point clouds to 1e-9 of the range."""
    from test_oracle_golden import NP2_CASES, NP2_SEEDS, YAML_OS2D, YAML_SEQ, np2_cfg_text
    g = np.load(os.path.join(GOLDEN, "detectors_np2.npz"))
    for cfg, shape, az, el in NP2_CASES:
        cm = make_cm(np2_cfg_text(cfg))
        tag = "x".join(str(x) for x in shape)
        pcg = PointCloudGenerator(cm, az_antenna_idxs=az, el_antenna_idxs=el,
                                  detector_params={"cfar_type": "ca_cfar_2d",
                                                   "cfar_params": {"num_train": (4, 4), "num_guard": (2, 2), "pfa": 1e-5}})
        os2d = RangeDopplerDetector2D(cm, cfar_type="os_cfar_2d", cfar_params=dict(YAML_OS2D))
        seq = RangeDopplerDetectorSequential(cm, rng_cfar_type=YAML_SEQ[0], rng_cfar_params=YAML_SEQ[1], vel_cfar_type=YAML_SEQ[2],
                                             vel_cfar_params=YAML_SEQ[3])
        for seed in NP2_SEEDS:
            cube = synth.synth_cube(seed, shape)
            pc = pcg.process(cube)
            np.testing.assert_array_equal(pcg.detector.dets, g[f"{tag}_s{seed}_dets"])
            np.testing.assert_allclose(pc, g[f"{tag}_s{seed}_pc"], rtol=0, atol=1e-9 * cm.range_max_m)
            np.testing.assert_array_equal(os2d.process(cube), g[f"{tag}_s{seed}_os2d"])
            np.testing.assert_array_equal(seq.process(cube), g[f"{tag}_s{seed}_seq"])


def test_ground_detector_and_altimeter_match_reference_fixtures():
    """RangeDopplerGroundDetector (stateful Altimeter gate) over the 5-frame sequence, reset(), and through
    PointCloudGenerator(detector_type="range_doppler_ground_detector") -- detections, altitude track and point clouds of the
    reference."""
    from mmwave_radar_processing_amd.processors.range_doppler_detection import RangeDopplerGroundDetector
    g = np.load(os.path.join(GOLDEN, "detectors_rd.npz"))
    cm = make_cm(synth.SYNTH_CFG_256x128x12)
    seq = synth.synth_ground_sequence(606, 5)
    for name, (vel_kind, vel_params, alt_params) in GROUND.items():
        det = RangeDopplerGroundDetector(cm, vel_cfar_type=vel_kind, vel_cfar_params=vel_params, altimeter_params=alt_params)
        track = []
        for f in range(5):
            np.testing.assert_array_equal(det.process(seq[f]), g[f"ground_{name}_f{f}"])
            track.append(det.altimeter.current_altitude_corrected_m)
        # (zoom bins are a linspace over the search window: the float32 chirp-z transform picks the reference's bin)
        np.testing.assert_allclose(track, g[f"ground_{name}_alt"], rtol=0, atol=1e-9)
        det.reset()
        np.testing.assert_array_equal(det.process(seq[3]), g[f"ground_{name}_after_reset_f3"])
        np.testing.assert_allclose(det.altimeter.current_altitude_corrected_m, g[f"ground_{name}_after_reset_alt"], rtol=0, atol=1e-9)
    vel_kind, vel_params, alt_params = GROUND["precise"]
    pcg = PointCloudGenerator(cm, az_antenna_idxs=[0, 3, 4, 7], el_antenna_idxs=[9, 8, 5, 4],
                              detector_type="range_doppler_ground_detector",
                              detector_params=dict(vel_cfar_type=vel_kind, vel_cfar_params=vel_params, altimeter_params=alt_params))
    sc = O.cfg_scalars(synth.SYNTH_CFG_256x128x12)
    for f in range(3):
        np.testing.assert_allclose(pcg.process(seq[f]), g[f"ground_pc_f{f}"], rtol=0, atol=1e-9 * sc["range_max_m"])


def test_non_finite_sample_in_an_end_antenna_is_the_one_documented_divergence(monkeypatch):
    """The reference's 3-D chain returns NaN everywhere when ANY antenna holds an inf sample -- also an end antenna, whose
    Hann(12) weight is exactly 0 (0 * inf = NaN; fixture inf_ant0 / inf_ant5).  The angle kernels never LOAD the two
    zero-weight planes (and mmw_chain3d(d_rd = NULL) does not even transform them), so an inf in antenna 0 or 11 leaves the
    output FINITE and equal to the clean cube's; with the inf in a live antenna, or with MMW_ANGLE_ZE=0
    MMW_CHAIN_SKIP_ENDS=0, nothing is finite, like the reference's."""
    g = np.load(os.path.join(GOLDEN, "detectors_rd.npz"))
    assert int(g["inf_ant0_finite_count"]) == 0 and int(g["inf_ant5_finite_count"]) == 0
    ctx = _lib.default_context()
    V, S, C, A = 12, 256, 128, 64
    d_in, d_out, d_rd = ctx.alloc(V * S * C * 8), ctx.alloc(A * S * C * 8), ctx.alloc(V * S * C * 8)

    def run(ant, keep_rd=False):
        cube = synth.synth_cube(3).copy()
        cube[ant, 17, 9] = np.inf
        d_in.upload(cube)
        _lib.check(ctx.lib.mmw_chain3d(ctx.handle, d_in.ptr, d_rd.ptr if keep_rd else None, d_out.ptr, 1, V, S, C, A, 0))
        return int(np.isfinite(d_out.download((A, S, C), np.complex64)).sum())

    assert run(5) == 0                              # live antenna: nothing finite, as in the reference
    assert run(0, keep_rd=True) == A * S * C        # the divergence: the end planes are transformed here, but never read
    assert run(0) == A * S * C                      # ... and here not even transformed
    ref = O.fft3d_windowed(synth.synth_cube(3), A)
    cube = synth.synth_cube(3).copy()
    cube[0, 17, 9] = np.inf
    d_in.upload(cube)
    _lib.check(ctx.lib.mmw_chain3d(ctx.handle, d_in.ptr, None, d_out.ptr, 1, V, S, C, A, 0))
    assert rel_err(d_out.download((A, S, C), np.complex64), ref) <= SPEC_TOL        # ... and equals the clean cube's result
    # the two switches of this context restore the reference's behaviour: every plane transformed and loaded, 0 * inf = NaN
    ctx.set_option("MMW_CHAIN_SKIP_ENDS", 0)
    ctx.set_option("MMW_ANGLE_ZE", 0)
    try:
        _lib.check(ctx.lib.mmw_chain3d(ctx.handle, d_in.ptr, None, d_out.ptr, 1, V, S, C, A, 0))
        assert int(np.isfinite(d_out.download((A, S, C), np.complex64)).sum()) == 0
    finally:
        ctx.set_option("MMW_CHAIN_SKIP_ENDS", None)
        ctx.set_option("MMW_ANGLE_ZE", None)
    for b in (d_in, d_out, d_rd):
        b.free()


def test_frame_pipeline_stream_overlaps_uploads_and_matches_load():
    """FramePipeline.stream: host chunks (complex64, pinned complex64, int16 raw) through the double-buffered upload give the
    results of load() + point_clouds() chunk by chunk, ragged last chunk included."""
    from mmwave_radar_processing_amd.batch import FramePipeline
    cm = make_cm(synth.synth_cfg_text(num_samples=64, num_loops=32))
    shape, az, el = (12, 64, 32), list(range(8)), [8, 9, 10, 11]
    cubes = np.stack([synth.synth_cube(9100 + f, shape) for f in range(11)])
    chunks = [cubes[0:4], cubes[4:8], cubes[8:11]]
    cfar = CaCFAR2D((4, 4), (2, 2), 1e-3)
    ref_pipe = FramePipeline(cm, max_frames=4, shape=shape, cfar=cfar, az_antenna_idxs=az, el_antenna_idxs=el)
    ref = []
    for c in chunks:
        ref_pipe.load(c)
        ref.append(ref_pipe.point_clouds())
    pipe = FramePipeline(cm, max_frames=4, shape=shape, cfar=cfar, az_antenna_idxs=az, el_antenna_idxs=el)
    got = list(pipe.stream(chunks))
    assert len(got) == 3 and [len(g) for g in got] == [4, 4, 3]
    for g, r in zip(got, ref):
        for a, b in zip(g, r):
            np.testing.assert_array_equal(a, b)
    # chunks that already live in pinned memory
    pinned = pipe.ctx.host_array(cubes.shape, np.complex64)
    pinned[...] = cubes
    got2 = list(pipe.stream([pinned[0:4], pinned[4:8], pinned[8:11]], pinned=True))
    for g, r in zip(got2, ref):
        for a, b in zip(g, r):
            np.testing.assert_array_equal(a, b)
    # int16 I/Q raw chunks (layout not pinned by the reference): same detections as the complex64 cubes they encode
    nrx, ntx = 4, 3
    raw = np.empty((11, nrx, 64, ntx * 32), dtype=np.complex64)
    for t in range(ntx):
        raw[:, :, :, t::ntx] = cubes[:, t * nrx:(t + 1) * nrx]
    iq = np.stack([raw.real, raw.imag], axis=-1).astype(np.int16)
    got3 = list(pipe.stream([iq[0:4], iq[4:8], iq[8:11]], num_tx=ntx))
    for g, r in zip(got3, ref):
        for a, b in zip(g, r):
            np.testing.assert_array_equal(a, b)
    # a custom work function: detections only
    got4 = list(pipe.stream(chunks, work=lambda p: p.detect()))
    assert [len(g) for g in got4] == [4, 4, 3] and got4[2][2].dtype == np.int64


@pytest.mark.parametrize("nrx,ntx,S,C", [(4, 3, 256, 128), (4, 3, 63, 100), (4, 2, 254, 50), (4, 3, 64, 32), (2, 2, 16, 8),
                                         (4, 3, 512, 64)])
def test_int16_raw_cubes_folded_into_the_first_kernel(nrx, ntx, S, C, monkeypatch):
    """mmw_range_doppler_raw_i16 / mmw_chain3d_raw_i16 (int16 I/Q cells converted and de-interleaved inside the loads of the
    first kernel; NO UPSTREAM ORACLE for the layout) == mmw_virtual_array_reformat_i16 followed by the virtual-array entry
    point, bit for bit, and within the spectrum tolerance of the oracle on the de-interleaved cube."""
    ctx = _lib.default_context()
    F, V, A = 5, nrx * ntx, 64
    rng = np.random.default_rng(S * 1000 + C)
    iq = rng.integers(-2000, 2000, size=(F, nrx, S, ntx * C, 2), dtype=np.int16)
    d_iq, d_virt = ctx.alloc(iq.nbytes), ctx.alloc(F * V * S * C * 8)
    d_a, d_b = ctx.alloc(F * V * S * C * 8), ctx.alloc(F * V * S * C * 8)
    d_iq.upload(iq)
    L, h = ctx.lib, ctx.handle
    _lib.check(L.mmw_virtual_array_reformat_i16(h, d_iq.ptr, d_virt.ptr, F, nrx, ntx, S, C))
    _lib.check(L.mmw_range_doppler(h, d_virt.ptr, d_a.ptr, None, F, V, S, C))
    _lib.check(L.mmw_range_doppler_raw_i16(h, d_iq.ptr, d_b.ptr, F, nrx, ntx, S, C))
    a, b = d_a.download((F, V, S, C), np.complex64), d_b.download((F, V, S, C), np.complex64)
    np.testing.assert_array_equal(a, b)
    virt = d_virt.download((F, V, S, C), np.complex64)
    assert rel_err(b[2], O.range_doppler(virt[2])) <= SPEC_TOL
    # the 3-D chain
    d_o1, d_o2 = ctx.alloc(F * A * S * C * 8), ctx.alloc(F * A * S * C * 8)
    _lib.check(L.mmw_chain3d(h, d_virt.ptr, None, d_o1.ptr, F, V, S, C, A, 0))
    _lib.check(L.mmw_chain3d_raw_i16(h, d_iq.ptr, None, d_o2.ptr, F, nrx, ntx, S, C, A, 0))
    o1, o2 = d_o1.download((F, A, S, C), np.complex64), d_o2.download((F, A, S, C), np.complex64)
    assert cross_schedule_dev(o1, o2) <= CROSS_SCHEDULE_TOL
    # several chunks per call, serial and overlapped schedules (the input of chunk k starts k * chunk * 4-byte-cell frames in)
    for pipe in ("0", "1"):
        monkeypatch.setenv("MMW_CHAIN_CHUNK", "2")
        monkeypatch.setenv("MMW_CHAIN_PIPELINE", pipe)
        d_o2.zero()
        _lib.check(L.mmw_chain3d_raw_i16(h, d_iq.ptr, None, d_o2.ptr, F, nrx, ntx, S, C, A, 0))
        assert cross_schedule_dev(o1, d_o2.download((F, A, S, C), np.complex64)) <= CROSS_SCHEDULE_TOL
    monkeypatch.delenv("MMW_CHAIN_CHUNK")
    if (S, C) == (256, 128):
        # the device-synchronised schedule (int16 variant of the persistent 256 x 128 producer), larger batch, twice in a row
        F2 = 150
        iq2 = rng.integers(-2000, 2000, size=(F2, nrx, S, ntx * C, 2), dtype=np.int16)
        d_iq2, d_v2 = ctx.alloc(iq2.nbytes), ctx.alloc(F2 * V * S * C * 8)
        d_p, d_q = ctx.alloc(F2 * A * S * C * 8), ctx.alloc(F2 * A * S * C * 8)
        d_iq2.upload(iq2)
        _lib.check(L.mmw_virtual_array_reformat_i16(h, d_iq2.ptr, d_v2.ptr, F2, nrx, ntx, S, C))
        monkeypatch.setenv("MMW_CHAIN_PIPELINE", "0")
        _lib.check(L.mmw_chain3d(h, d_v2.ptr, None, d_p.ptr, F2, V, S, C, A, 0))
        monkeypatch.setenv("MMW_CHAIN_PIPELINE", "1")
        plan = (_lib.C.c_int * 8)()
        _lib.check(L.mmw_diag_chain_plan(h, F2, V, S, C, A, 0, plan))
        assert plan[6] == 1
        for _ in range(2):
            _lib.check(L.mmw_chain3d_raw_i16(h, d_iq2.ptr, None, d_q.ptr, F2, nrx, ntx, S, C, A, 0))
        picks = [0, 71, 149]
        p_ = np.stack([d_p.download((A, S, C), np.complex64, f * A * S * C * 8) for f in picks])
        q_ = np.stack([d_q.download((A, S, C), np.complex64, f * A * S * C * 8) for f in picks])
        assert cross_schedule_dev(p_, q_) <= CROSS_SCHEDULE_TOL
        _lib.check(L.mmw_diag_chain_plan(h, F2, V, S, C, A, 0, plan))
        assert plan[5] == 0             # no hand-off timeout, nothing re-run
        for buf in (d_iq2, d_v2, d_p, d_q):
            buf.free()
    monkeypatch.delenv("MMW_CHAIN_PIPELINE")
    assert rel_err(o2[4], O.fft3d_windowed(virt[4], A)) <= SPEC_TOL
    for buf in (d_iq, d_virt, d_a, d_b, d_o1, d_o2):
        buf.free()
