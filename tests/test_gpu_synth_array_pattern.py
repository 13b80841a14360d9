"""mmw_synth_array_pattern on the device: the reference-generated fixture through ``batch.array_patterns`` under both bounds of
``synth_pattern_cases`` (E = 102, 65 and 33 are no multiples of the wave size; T = 257 goes past one workgroup's threads and one
direction tile); exact ones, the NaN frame, bit-identical repeats, the device against the host-only twin (also with E past one LDS
chunk), guards behind the outputs and refusals that write nothing; the mirrored class, ``batch.synthetic_array_patterns`` and
``FramePipeline.synthetic_array_patterns`` with and without calibration, with the host route of the calibration forced, and with
no valid frame at all."""
import ctypes

import numpy as np
import pytest

from mmwave_radar_processing_amd import _lib, batch
from mmwave_radar_processing_amd.batch import FramePipeline
from mmwave_radar_processing_amd.processors import SelfCalibratingSyntheticArrayProcessor, SyntheticArrayBeamformerProcessor
from synth_pattern_cases import PATTERN_TOL, SETS, af_bound, check, directions, fixture_set, host_patterns, nan_case
from test_synth_array_calib_host import case_processor
from test_synth_array_host import fixture_processor

pytestmark = pytest.mark.gpu


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.float64)


@pytest.mark.parametrize("name", SETS)
def test_fixture_sets_under_both_bounds(golden, name):
    P, d, lam, want_pattern, want_af = fixture_set(golden("synth_array_pattern.npz"), name)
    pat, af = batch.array_patterns(P, d, lam, with_factor=True)
    check(f"device, set {name}", pat, af, want_pattern, want_af, af_bound(P, d, lam))
    # without the array factor: the same patterns; and the same call again: the same bits
    assert np.array_equal(bits(batch.array_patterns(P, d, lam)), bits(pat))
    again, again_af = batch.array_patterns(P, d, lam, with_factor=True)
    assert np.array_equal(bits(again), bits(pat)) and np.array_equal(bits(again_af), bits(af))


def test_zero_geometry_and_one_element_give_exact_ones():
    d = directions(67, 3)
    pat, af = batch.array_patterns(np.zeros((2, 3, 130)), d, 0.0039, with_factor=True)
    assert (pat == 1.0).all() and (af == 130.0).all()
    rng = np.random.default_rng(3)
    pat, af = batch.array_patterns(rng.uniform(-2, 2, (4, 3, 1)), d, 0.0039, with_factor=True)
    assert (pat == 1.0).all() and np.abs(np.abs(af) - 1.0).max() <= 2.0 ** -51


def test_nan_frame_is_all_nan_and_leaves_the_others_alone():
    P, bad, d, lam = nan_case()
    clean, clean_af = batch.array_patterns(P, d, lam, with_factor=True)
    got, got_af = batch.array_patterns(bad, d, lam, with_factor=True)
    assert np.isnan(got[1]).all() and np.isnan(got_af[1]).all() and np.isfinite(clean).all()
    for i in (0, 2):
        assert np.array_equal(bits(got[i]), bits(clean[i])) and np.array_equal(bits(got_af[i]), bits(clean_af[i]))


@pytest.mark.parametrize("name", SETS + ("two LDS chunks",))
def test_device_and_host_entry_agree(golden, name):
    if name in SETS:
        P, d, lam, _, _ = fixture_set(golden("synth_array_pattern.npz"), name)
    else:       # E past one chunk of the kernel's LDS staging and no multiple of anything; the second direction tile holds one direction
        P, d, lam = np.random.default_rng(11).uniform(-0.3, 0.3, (2, 3, 2061)), directions(11, 3), 0.0039
        # the host twin has no chunks; numpy's own sum says it is right at this size too
        ref = np.exp(2j * np.pi * np.einsum("cat,nce->nate", d, P) / lam).sum(-1)
        assert (np.abs(host_patterns(P, d, lam)[1] - ref) <= af_bound(P, d, lam)).all()
    want_pattern, want_af = host_patterns(P, d, lam)
    pat, af = batch.array_patterns(P, d, lam, with_factor=True)
    check(f"device against the host entry, {name}", pat, af, want_pattern, want_af, af_bound(P, d, lam))


def test_guards_refusals_and_the_profile_family(golden):
    P, d, lam, want_pattern, _ = fixture_set(golden("synth_array_pattern.npz"), "b")
    P = np.ascontiguousarray(P[:2])
    n, E, T, guard = 2, P.shape[2], d.shape[1] * d.shape[2], 64
    dirs = np.ascontiguousarray(d.reshape(3, -1))
    ctx = _lib.default_context()
    d_P, d_pat, d_af = ctx.alloc(P.nbytes), ctx.alloc((n * T + guard) * 4), ctx.alloc((n * T + guard) * 16)
    dp = ctypes.POINTER(ctypes.c_double)

    def call(**over):
        a = dict(P=d_P.ptr, n=n, E=E, dirs=dirs.ctypes.data_as(dp), T=T, lam=lam, pat=d_pat.ptr)
        a.update(over)
        return ctx.lib.mmw_synth_array_pattern(ctx.handle, a["P"], a["n"], a["E"], a["dirs"], a["T"], a["lam"], a["pat"], d_af.ptr)
    try:
        d_P.upload(P)
        d_pat.upload(np.full(n * T + guard, -7.0, dtype=np.float32))
        d_af.upload(np.full(n * T + guard, -7.0, dtype=np.complex128))
        for over in (dict(P=None), dict(dirs=None), dict(pat=None), dict(n=-1), dict(E=0), dict(T=0), dict(lam=0.0), dict(lam=float("inf")),
                     dict(lam=float("nan")), dict(n=2**16, T=2**15)):
            assert call(**over) == _lib.MMW_ERR_INVALID, over
        assert call(n=0) == _lib.MMW_OK
        assert (d_pat.download((n * T + guard,), np.float32) == -7.0).all() and (d_af.download((n * T + guard,), np.complex128) == -7.0).all()
        ctx.profile_reset()
        ctx.profile_enable(True)
        try:
            _lib.check(call())
            ms, launches = ctx.profile_get("synth_pattern")
        finally:
            ctx.profile_enable(False)
        assert launches == 1 and ms > 0.0
        pat, af = d_pat.download((n * T + guard,), np.float32), d_af.download((n * T + guard,), np.complex128)
    finally:
        for b in (d_P, d_pat, d_af):
            b.free()
    assert (pat[n * T:] == -7.0).all() and (af[n * T:] == -7.0).all(), "guard overwritten"
    assert np.abs(pat[:n * T].reshape(n, *d.shape[1:]) - want_pattern[:2]).max() <= PATTERN_TOL


def test_mirrored_class_equals_the_fixture(golden):
    g = golden("synth_array_pattern.npz")
    p = fixture_processor(golden("synth_array.npz"))
    got = np.stack([p.compute_synthetic_array_pattern(geo) for geo in g["a_geometry"]])
    check("SyntheticArrayBeamformerProcessor.compute_synthetic_array_pattern, set a", got, None, g["a_pattern"], None, None)
    assert got[0].shape == (7, 2)
    assert SelfCalibratingSyntheticArrayProcessor.compute_synthetic_array_pattern is SyntheticArrayBeamformerProcessor.compute_synthetic_array_pattern


def test_patterns_of_a_velocity_sequence(golden):
    g, s = golden("synth_array_pattern.npz"), golden("synth_array.npz")
    p = fixture_processor(s)
    frames, pat = batch.synthetic_array_patterns(p, s["velocities"])
    assert frames.tolist() == [2, 3, 7] and frames.dtype == np.int64
    check("batch.synthetic_array_patterns", pat, None, g["a_pattern"][[2, 3, 7]], None, None)
    # velocities that open no gate: empty arrays of the right shape
    frames, pat = batch.synthetic_array_patterns(p, np.zeros((5, 3)))
    assert frames.shape == (0,) and pat.shape == (0, 7, 2) and pat.dtype == np.float32


def test_pipeline_patterns_with_and_without_calibration(golden, monkeypatch):
    g = golden("synth_array_calib.npz")
    proc = case_processor(g, "a", cls=SyntheticArrayBeamformerProcessor)
    n_it, vel = int(g["a_iters"]), g["velocities"]
    n, _, S, L = g["slabs"].shape
    cubes = np.zeros((n, 12, S, L), dtype=np.complex64)
    cubes[:, [int(a) for a in g["live"]]] = g["slabs"]
    fp = FramePipeline(proc.config_manager, max_frames=n, shape=(12, S, L))
    calibrations = []
    run = fp.synthetic_array_calibrated_device
    monkeypatch.setattr(fp, "synthetic_array_calibrated_device", lambda *a, **k: calibrations.append(1) or run(*a, **k))
    try:
        fp.load(cubes)
        # not calibrated: the module function on the pipeline's context
        frames, plain = fp.synthetic_array_patterns(proc, vel)
        want_frames, want = batch.synthetic_array_patterns(proc, vel, ctx=fp.ctx)
        assert frames.tolist() == want_frames.tolist() == g["a_frames"].tolist() and np.array_equal(bits(plain), bits(want))
        assert not calibrations
        # calibrated: runs the calibration once, reads its geometries in place
        frames, cal = fp.synthetic_array_patterns(proc, vel, calibrated=True, num_calibration_iters=n_it)
        assert frames.tolist() == g["a_frames"].tolist() and len(calibrations) == 1 and fp.n_flagged == 0
        assert (fp.synth_calib_status > 0).any()
        assert np.array_equal(bits(cal), bits(batch.array_patterns(fp.synth_geometry_calibrated, proc.d, proc.lambda_m, ctx=fp.ctx)))
        assert any(not np.array_equal(cal[i], plain[i]) for i in range(len(frames)))
        # the calibrated images of these arguments are resident: no second calibration; the device twin leaves the table in HBM
        frames2, buf = fp.synthetic_array_patterns_device(proc, vel, calibrated=True, num_calibration_iters=n_it)
        assert len(calibrations) == 1 and frames2.tolist() == frames.tolist()
        assert np.array_equal(bits(buf.download(cal.shape, np.float32)), bits(cal))
        # other arguments, or other cubes, are not: the calibration runs again
        fp.synthetic_array_patterns(proc, vel, calibrated=True, num_calibration_iters=n_it + 1)
        assert len(calibrations) == 2
        # every frame through the host route: the corrected rows are uploaded before the kernel reads the table
        fp.ctx.set_option("MMW_SYNTH_CALIB_FLAG_ALL", 1)
        try:
            fp.load(cubes)
            frames, cal_host = fp.synthetic_array_patterns(proc, vel, calibrated=True, num_calibration_iters=n_it)
        finally:
            fp.ctx.set_option("MMW_SYNTH_CALIB_FLAG_ALL", None)
        assert len(calibrations) == 3 and fp.n_flagged == len(frames) == 3 and (fp.synth_calib_status > 0).any()
        assert np.array_equal(bits(cal_host), bits(batch.array_patterns(fp.synth_geometry_calibrated, proc.d, proc.lambda_m, ctx=fp.ctx)))
        assert np.abs(cal_host - cal).max() <= PATTERN_TOL          # (the two routes agree on the geometry to rounding)
        # no valid frame: empty arrays of the right shape, calibrated or not
        for calibrated in (False, True):
            frames, none = fp.synthetic_array_patterns(proc, np.zeros((n, 3)), calibrated=calibrated)
            assert frames.shape == (0,) and none.shape == (0,) + proc.d.shape[1:] and none.dtype == np.float32
    finally:
        fp.bufs.free()
