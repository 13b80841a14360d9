"""``mmw_doppler_azimuth_ransac`` on the device: rows and flags bit-identical to the host-only entry (one rule, two realisations of
a wave) on every crafted list of tests/golden/dopaz_velocity.npz and on random lists, the recorded reference values, launches
whose last workgroup is partly empty, ``FramePipeline.doppler_azimuth_fits`` / ``doppler_azimuth_velocities`` and the mirrored class
on the two recorded sequences against the reference class's recorded tracks, state across calls, ``stream()`` chunks and the
multi-device form, and the maps and peak tables left untouched.  The kernel tests need no scikit-learn: the tables are stored."""
import json
import os

import numpy as np
import pytest

import dopaz_velocity_cases as K
from mmwave_radar_processing_amd import _lib, synth
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline
from mmwave_radar_processing_amd.config_managers import ConfigManager

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return K.fixture()


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


def _same(dev, host_out, host_flags):
    out, flags = dev
    assert np.array_equal(flags, host_flags)
    assert np.array_equal(out.view(np.uint64), host_out.view(np.uint64))       # bit for bit, signed zeros included


@pytest.mark.parametrize("per_frame", [True, False])
@pytest.mark.parametrize("G", [1, 2])
def test_kernel_equals_the_host_entry_and_the_reference_on_every_crafted_list(ctx, fx, per_frame, G):
    theta, cases, rel_tol = fx
    seen = set()
    for n_rows, row, zero, vel, group in K.batches(cases, theta, per_frame):
        assert row.shape[1] <= 40
        seen.add(n_rows)
        row, zero = np.repeat(row, G, axis=0), np.repeat(zero, G, axis=0)
        rc, h_out, h_flags = K.host_call(row, zero, vel, theta)
        assert rc == 0
        dev = K.run_device_entry(ctx, row, zero, vel, theta)
        _same(dev, h_out, h_flags)
        bits, status, inliers = K.decode(dev[1])
        for g in range(G):
            for f, case in enumerate(group):
                K.check_against_reference(case, dev[0][g, f], bits[g, f], status[g, f], inliers[g, f], rel_tol)
                assert not (case.clear and bits[g, f]), case.name
    assert seen == {12, 64, 65, 100, 128, 200, 256}


@pytest.mark.parametrize("branch,F,G", [("std", 41, 1), ("small", 41, 1), ("std", 200, 2), ("small", 3, 1)])
def test_partly_empty_last_workgroup_and_random_lists(ctx, fx, branch, F, G):
    """4 k + 1 and 4 k + 3 pairs: the last workgroup's spare waves leave; m[f] cuts frames short; two groups share vx."""
    theta = fx[0]
    row, zero, vel = K.random_lists(theta, branch, count=F)
    row, zero = np.repeat(row, G, axis=0), np.repeat(zero, G, axis=0)
    if G == 2:
        row[1] = row[1, ::-1]
    m = np.full(F, row.shape[2], dtype=np.int32)
    m[::7] = 90
    m[1] = 0
    zero[:, m <= zero.max(axis=0)] = -1
    kw = dict(m=m, g_az=0, g_el=G - 1 if G == 2 else -1)
    rc, h_out, h_flags = K.host_call(row, zero, vel, theta, **kw)
    assert rc == 0
    _same(K.run_device_entry(ctx, row, zero, vel, theta, **kw), h_out, h_flags)
    bits, status, _ = K.decode(h_flags)
    assert status[0, 1] == K.EMPTY and np.count_nonzero(bits) * 10 <= bits.size


def test_decision_lists_are_flagged_on_the_device_as_on_the_host(ctx, fx):
    theta = fx[0]
    for (row, zero, vel), bit in ((K.residual_at_threshold(theta), _lib.DOPAZ_FLAG_RESIDUAL),
                                  (K.mirrored_trials(theta), _lib.DOPAZ_FLAG_SCORE_TIE)):
        rc, h_out, h_flags = K.host_call(row[None, None], [[zero]], vel, theta)
        dev = K.run_device_entry(ctx, row[None, None], [[zero]], vel, theta)
        _same(dev, h_out, h_flags)
        assert K.decode(dev[1])[0][0, 0] & bit and np.all(dev[0] == 0.0)
    only = K.run_device_entry(ctx, row[None, None], [[zero]], vel, theta, mode=_lib.DOPAZ_RANSAC_VX_ONLY)
    assert only[1][0, 0] == 0 and only[0][0, 0, 0] == -1 * vel[zero] and np.all(only[0][0, 0, 1:] == 0.0)


# ------------------------------------------------------------------------------------------------ the pipeline
def _estimator(name, **kw):
    from mmwave_radar_processing_amd.processors.velocity_estimator import VelocityEstimator
    cm = ConfigManager()
    if name == "standard":
        cm.load_cfg_text(synth.synth_cfg_text(num_samples=64, num_loops=32))
        shape = (12, 64, 32)
    else:
        with open(os.path.join(GOLDEN, "cfg_scalars.json")) as f:
            cm.load_cfg_text("\n".join(json.load(f)["6843_RadVel_ods_20Hz.cfg"]["lines"]), array_geometry="ods")
        shape = (12, 63, 70)
    return VelocityEstimator(cm, lower_range_bound=0.5, upper_range_bound=1.5, peak_threshold_dB=25.0, **kw), shape


def _scene(name, shape, F, first=0):
    """Frames ``first .. F - 1`` of the moving-platform sequence of one geometry (made from the seed, as every call makes it)."""
    cm = _estimator(name)[0].config_manager
    vel = None
    if name == "standard":                   # 0.3 m/s velocity bins: a faster platform
        vel = np.stack([1.2 + 0.15 * np.arange(F), -1.5 + 0.3 * np.arange(F)], axis=1)
    cubes, _ = synth.synth_moving_platform_sequence(77, F, shape, cm.range_res_m, cm.vel_res_m_s, name, (1.1, 2.9), vel)
    return cubes[first:]


def _host_route(pipe, est, altitudes, precise):
    """The fits by the route that needs no new kernel: ``doppler_azimuth_peaks`` (coarse, then precise) and the host-only entry
    on index tables rebuilt from its peak lists."""
    from mmwave_radar_processing_amd.batch import precise_ranges_from_zero_az
    from mmwave_radar_processing_amd.processors.velocity_estimator import antenna_plan
    cm = est.config_manager
    sets, groups, shift = antenna_plan(cm)
    win = np.stack([est.get_range_window(altitude=a, sensing_direction=cm.array_direction) for a in altitudes])
    pv = None
    if precise:
        _, zero_az = pipe.doppler_azimuth_peaks(est, sets, groups, win, shift, None, est.peak_threshold_dB)
        pv = precise_ranges_from_zero_az(zero_az[0], zero_az[1] if len(groups) == 2 else None, est.precise_vel_bound)
    row, zero, m, bins = pipe.doppler_azimuth_peaks_device(est, sets, groups, win, shift, pv, est.peak_threshold_dB)
    F = len(altitudes)
    if m is None:
        vel = np.asarray(est.vel_bins, dtype=np.float64)
    else:
        vel = np.zeros((F, row.shape[2]))
        for f in range(F):
            vel[f, :m[f]] = bins[f]
    rc, out, flags = K.host_call(row, zero, vel, est.valid_angle_bins, m=m, g_az=0, g_el=1 if len(groups) == 2 else -1,
                                 mode=_lib.DOPAZ_RANSAC_VX_ONLY if est.x_measurement_only else 0, min_r2=est.min_R2_threshold,
                                 min_share=est.min_inlier_percent)
    assert rc == 0
    return out.transpose(1, 0, 2), flags.T


@pytest.mark.parametrize("name", ["standard", "ods"])
@pytest.mark.parametrize("precise", [False, True])
def test_pipeline_fits_equal_the_peaks_route_and_leave_its_tables_alone(name, precise):
    est, shape = _estimator(name)
    F = 9
    pipe = FramePipeline(est.config_manager, max_frames=F, shape=shape)
    pipe.load(_scene(name, shape, F))
    alt = np.linspace(1.4, 1.6, F)
    want, want_flags = _host_route(pipe, est, alt, precise)
    d_maps, map_shape = pipe.dopaz_peak_maps
    d_row, d_zero = pipe.bufs.get("dopaz_row_peak", 4), pipe.bufs.get("dopaz_zero_peak", 4)
    before = [d_maps.download(map_shape, np.float32).copy(), d_row.download((d_row.nbytes,), np.uint8).copy(),
              d_zero.download((d_zero.nbytes,), np.uint8).copy()]
    fits, status = pipe.doppler_azimuth_fits(est, alt, enable_precise_responses=precise)
    after = [d_maps.download(map_shape, np.float32), d_row.download((d_row.nbytes,), np.uint8), d_zero.download((d_zero.nbytes,), np.uint8)]
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()                                    # the maps and the peak tables: byte for byte
    bits, want_status, _ = K.decode(want_flags)
    decided = bits == 0
    print(name, precise, "flag bits per (frame, group):", bits.ravel().tolist(), "status:", want_status.ravel().tolist())
    assert fits.shape == want.shape == (F, want.shape[1], 4) and status.shape == decided.shape
    assert np.array_equal(fits[decided].view(np.uint64), want[decided].view(np.uint64))
    assert np.array_equal(status[decided], want_status[decided])
    assert pipe.n_dopaz_fits_flagged == np.count_nonzero(~decided) and pipe.n_dopaz_fits_flagged * 10 <= decided.size


# ------------------------------------------------------------------------------------------------ the recorded sequences
def _recorded_setup(name):
    from mmwave_radar_processing_amd.processors.velocity_estimator import VelocityEstimator
    text, kw, shape, F = K.sequence_cfg(name)
    cm = ConfigManager()
    cm.load_cfg_text(text, **kw)
    return cm, shape, F, (lambda: VelocityEstimator(cm, **K.ESTIMATOR_KW))


_scenes = {}


def _recorded_scene(name):
    """(cubes, altitudes), made once per geometry and never written to."""
    if name not in _scenes:
        cm = _recorded_setup(name)[0]
        cubes, alt = K.sequence(name, cm.range_res_m, cm.vel_res_m_s)
        cubes.setflags(write=False)
        _scenes[name] = (cubes, alt)
    return _scenes[name]


def _gates(est_factory, fits, status):
    """Per frame and direction: did the fit pass the estimator's gates (R^2, and on ods the share)."""
    est = est_factory()
    ok = (fits[..., 2] >= est.min_R2_threshold)
    if est.config_manager.array_geometry == "ods":
        ok &= fits[..., 3] >= est.min_inlier_percent
    return ok


def _assert_track(label, got, track, rel_tol):
    want = track["current"]
    dev = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(label, "worst deviation of the current estimates from the recorded track:", float(dev.max()), "per frame:",
          np.round(dev.max(axis=1), 18).tolist())
    assert np.all((got == 0.0) == (want == 0.0)), label                     # the gate outcomes, component by component
    assert dev.max() <= rel_tol, (label, float(dev.max()))


@pytest.mark.parametrize("name", ["standard", "ods"])
@pytest.mark.parametrize("mode", ["coarse", "precise"])
def test_pipeline_tracks_equal_the_recorded_reference_tracks(fx, name, mode):
    """``doppler_azimuth_fits`` / ``doppler_azimuth_velocities`` on the recorded sequences against what the reference class's
    ``process`` gave frame by frame (tests/golden/dopaz_velocity.npz): the current estimates within ``rel_tol``, the gate outcomes
    identical, the flagged share within one pair in ten; then the same track from two calls that split the sequence, from
    ``stream()`` chunks and from the multi-device form on one device."""
    rel_tol = fx[2]
    cm, shape, F, make = _recorded_setup(name)
    cubes, alt = _recorded_scene(name)
    track = K.recorded(name, mode)
    precise = mode == "precise"
    pipe = FramePipeline(cm, max_frames=F, shape=shape)
    pipe.load(cubes)
    fits, status = pipe.doppler_azimuth_fits(make(), alt, precise)
    print(name, mode, "flagged pairs:", pipe.n_dopaz_fits_flagged, "of", status.size)
    assert pipe.n_dopaz_fits_flagged * 10 <= status.size
    want_status = K.recorded_status(track)
    fitted = (want_status == K.OK) & (status == K.OK)
    assert np.array_equal(status == K.EMPTY, want_status == K.EMPTY)
    assert np.array_equal(_gates(make, fits, status)[fitted], _gates(make, track["fits"], want_status)[fitted])
    whole = pipe.doppler_azimuth_velocities(make(), alt, precise)
    _assert_track(f"{name} {mode}", whole, track, rel_tol)
    # state carries: two calls that split the sequence, stream() chunks, the multi-device form -- bit for bit the one-call track
    cut = 5
    est = make()
    pipe.load(cubes[:cut])
    first = pipe.doppler_azimuth_velocities(est, alt[:cut], precise)
    pipe.load(cubes[cut:])
    second = pipe.doppler_azimuth_velocities(est, alt[cut:], precise)
    assert np.array_equal(np.concatenate([first, second]), whole)
    est, bounds = make(), [(lo, min(lo + 7, F)) for lo in range(0, F, 7)]          # the last chunk is a short one
    nxt = iter(bounds)

    def work(p):
        lo, hi = next(nxt)
        return p.doppler_azimuth_velocities(est, alt[lo:hi], precise).copy()

    small = FramePipeline(cm, max_frames=7, shape=shape)
    streamed = np.concatenate(list(small.stream((cubes[lo:hi] for lo, hi in bounds), work=work)))
    assert np.array_equal(streamed, whole)
    mp = MultiDeviceFramePipeline(cm, max_frames=F, shape=shape, devices=[0])
    mp.load(cubes)
    assert np.array_equal(mp.doppler_azimuth_velocities(make(), alt, precise), whole)
    mp.close()


@pytest.mark.parametrize("name", ["standard", "ods"])
@pytest.mark.parametrize("mode", ["coarse", "precise"])
def test_mirrored_class_stepped_over_the_recorded_sequences(fx, name, mode):
    """``VelocityEstimator.process`` frame by frame (maps on the device, pickers and scikit-learn on the host) against the
    recorded reference: vx, both fits, the proposal and the current estimate of every frame."""
    pytest.importorskip("sklearn")
    import warnings
    rel_tol = fx[2]
    cm, shape, F, make = _recorded_setup(name)
    cubes, alt = _recorded_scene(name)
    track = K.recorded(name, mode)
    est = make()
    G = track["fits"].shape[1]
    cur, prop, fits = np.zeros((F, 3)), np.zeros((F, 3)), np.zeros((F, G, 4))
    for f in range(F):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cur[f] = est.process(adc_cube=cubes[f], altitude=alt[f], enable_precise_responses=mode == "precise")
        prop[f] = est.proposed_velocity_estimate
        fits[f, 0] = (est.ego_vx_estimate, est.azimuth_ego_vy_estimate, est.azimuth_estimate_R2, est.azimuth_inlier_percent)
        if G == 2:
            fits[f, 1] = (est.ego_vx_estimate, est.elevation_ego_vy_estimate, est.elevation_estimate_R2, est.elevation_inlier_percent)
    for label, got, want in (("fits", fits, track["fits"]), ("proposal", prop, track["proposal"])):
        dev = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        print(name, mode, label, "worst deviation:", float(dev.max()))
        assert dev.max() <= rel_tol, (label, float(dev.max()))
    _assert_track(f"{name} {mode} class", cur, track, rel_tol)
    est.update_history(estimated=cur[-1])
    assert len(est.history_R2_statistics) == len(est.history_inlier_statistics) == len(est.history_estimated) == 1


def test_x_measurement_only_runs_the_zero_azimuth_part():
    est, shape = _estimator("standard", x_measurement_only=True)
    pipe = FramePipeline(est.config_manager, max_frames=3, shape=shape)
    pipe.load(_scene("standard", shape, 3))
    fits, status = pipe.doppler_azimuth_fits(est, 1.5)
    want, _ = _host_route(pipe, est, np.full(3, 1.5), False)
    assert np.array_equal(fits, want) and np.all(fits[..., 1:] == 0.0) and np.all(status == K.OK)
    track = pipe.doppler_azimuth_velocities(est, 1.5)
    assert np.array_equal(track[:, 0], fits[:, 0, 0])
