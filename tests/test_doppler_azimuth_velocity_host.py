"""Host side of the Doppler-azimuth RANSAC stage (no device): the entries in the header and the ctypes table, the shared rule
through ``mmw_diag_doppler_azimuth_ransac_host`` against the reference class's recorded results and (scikit-learn present) the
mirrored class on random lists, the flags of decisions that rounding could turn, the ordered compaction, the arguments the
entries refuse, the state scan, and the entries under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program)."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import dopaz_velocity_cases as K
from conftest import ROOT
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import dopaz_state_scan

HEADER = os.path.join(ROOT, "include", "mmwgpu.h")
TAIL = ["G", "F", "n_rows", "h_m", "vel", "vel_len", "vel_per_frame", "cos", "sin", "theta", "n_cols", "subsets", "trials", "n_tab",
        "trials_len", "g_az", "g_el", "mode", "thr_standard", "thr_small_vx", "min_R2", "min_inlier_share"]


@pytest.fixture(scope="module")
def fx():
    return K.fixture()


def test_entries_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, pre in (("mmw_doppler_azimuth_ransac", "d_"), ("mmw_diag_doppler_azimuth_ransac_host", "h_")):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/mmwgpu.h"
        got = [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]
        body = [n if n in ("G", "F", "n_rows", "h_m") or not re.fullmatch(r"vel|cos|sin|theta|subsets|trials", n) else pre + n for n in TAIL]
        assert got == (["ctx"] if pre == "d_" else []) + [pre + "row_peak", pre + "zero"] + body + [pre + "out", pre + "flags"]
        assert name in _lib.EXPORTED and len(_lib._SIGNATURES[name]) == len(got)
    for macro, value in (("FLAG_RESIDUAL", 1), ("FLAG_SCORE_TIE", 2), ("FLAG_R2", 4), ("FLAG_SHARE", 8), ("FLAG_A_ZERO", 16),
                         ("FLAG_NONFINITE", 32), ("FLAG_UNDECIDED", 64), ("FLAG_TABLES", 128), ("STATUS_SHIFT", 8), ("STATUS_EMPTY", 1),
                         ("STATUS_FAILED", 2), ("INLIERS_SHIFT", 16), ("RANSAC_MAX_ROWS", 512), ("RANSAC_VX_ONLY", 1)):
        m = re.search(r"#define\s+MMW_DOPAZ_" + macro + r"\s+(\S+)", text)
        assert m and int(m.group(1), 0) == value == getattr(_lib, "DOPAZ_" + macro), macro
    assert re.search(r"#define\s+MMWGPU_ABI_VERSION\s+7\b", text) and _lib.ABI_VERSION == 7
    make = open(os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS = .*\bmmw_tu_dopaz_velocity\b", make, flags=re.M)
    assert re.search(r"^build/mmw_tu_dopaz_velocity\.o:.*-ffp-contract=off", make, flags=re.M)


def test_host_entry_equals_the_recorded_reference_on_every_crafted_list(fx):
    theta, cases, rel_tol = fx
    assert {c.status for c in cases} == {K.OK, K.EMPTY, K.FAILED}
    flagged = 0
    for per_frame in (True, False):
        for n_rows, row, zero, vel, group in K.batches(cases, theta, per_frame):
            out, bits, status, inliers = K.run_host_entry(row, zero, vel, theta)
            for f, case in enumerate(group):
                print(case.name, out[0, f], int(bits[0, f]), int(status[0, f]), int(inliers[0, f]))
                K.check_against_reference(case, out[0, f], bits[0, f], status[0, f], inliers[0, f], rel_tol)
                assert not (case.clear and bits[0, f]), case.name            # the clear lists flag nothing
                flagged += int(bits[0, f] != 0)
    assert flagged * 10 <= 2 * len(cases)                                       # at most one pair in ten over the whole fixture


def test_lists_built_to_sit_on_a_decision_are_flagged(fx):
    theta = fx[0]
    row, zero, vel = K.residual_at_threshold(theta)
    out, bits, status, _ = K.run_host_entry(row[None, None], [[zero]], vel, theta)
    assert bits[0, 0] & _lib.DOPAZ_FLAG_RESIDUAL and np.all(out == 0.0)
    vel2 = vel.copy()
    vel2[np.flatnonzero(row == np.argmin(np.abs(theta)))[-1]] -= 1e-9        # a nanometre per second off the threshold: decided
    assert K.run_host_entry(row[None, None], [[zero]], vel2, theta)[1][0, 0] == 0
    row, zero, vel = K.mirrored_trials(theta)
    out, bits, status, _ = K.run_host_entry(row[None, None], [[zero]], vel, theta)
    assert bits[0, 0] == _lib.DOPAZ_FLAG_SCORE_TIE and np.all(out == 0.0), bits
    # thresholds of the gates placed on the values a clear list produces
    case = next(c for c in fx[1] if c.name == "std_128")
    for kw, bit in ((dict(min_r2=case.r2), _lib.DOPAZ_FLAG_R2), (dict(min_share=case.share), _lib.DOPAZ_FLAG_SHARE)):
        _, bits, _, _ = K.run_host_entry(case.row[None, None], [[case.zero]], case.vel, theta, **kw)
        assert bits[0, 0] == bit, (kw, bits)
    # non-finite table entries and undecided inputs
    bad = np.cos(theta)
    bad[case.row.max()] = np.nan
    assert K.run_host_entry(case.row[None, None], [[case.zero]], case.vel, theta, cos=bad)[1][0, 0] == _lib.DOPAZ_FLAG_NONFINITE
    row = case.row.copy()
    row[5] = -2
    assert K.run_host_entry(row[None, None], [[case.zero]], case.vel, theta)[1][0, 0] == _lib.DOPAZ_FLAG_UNDECIDED
    assert K.run_host_entry(case.row[None, None], [[-2]], case.vel, theta)[1][0, 0] == _lib.DOPAZ_FLAG_UNDECIDED
    row[5] = len(theta)
    assert K.run_host_entry(row[None, None], [[case.zero]], case.vel, theta)[1][0, 0] == _lib.DOPAZ_FLAG_TABLES


def _class_fit(theta, vel, row, zero_az, zero_el=-1):
    from mmwave_radar_processing_amd.processors.velocity_estimator import VelocityEstimator
    est = VelocityEstimator.__new__(VelocityEstimator)
    none = np.empty(shape=(0, 2))
    est.azimuth_peak_zero_az = np.array([0.0, vel[zero_az]]) if zero_az >= 0 else none
    est.elevation_peak_zero_az = np.array([0.0, vel[zero_el]]) if zero_el >= 0 else none
    vx = est.estimate_ego_vx_velocity()
    rows = np.flatnonzero(row >= 0)
    if len(rows) == 0:
        return vx, None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return vx, est.lsq_fit_ego_vy_ransac(np.stack([theta[row[rows]], vel[rows]], axis=1))


def _check_against_class(theta, vel, row, zero, out, bits, status, inliers, rel_tol, m=None):
    if bits:
        assert np.all(out == 0.0)
        return 1
    r = row if m is None else np.where(np.arange(len(row)) < m, row, -1)
    vx, fit = _class_fit(theta, vel, r, zero)
    assert out[0] == vx and np.signbit(out[0]) == np.signbit(vx)
    if fit is None:
        assert status == K.EMPTY
    elif fit == (0.0, 0.0, 0.0):
        assert status == K.FAILED and np.all(out[1:] == 0.0)
    else:
        n = int(np.count_nonzero(r >= 0))
        assert status == K.OK and out[3] == fit[2] and inliers == round(fit[2] * n)
        assert abs(out[1] - fit[0]) <= rel_tol * max(1.0, abs(fit[0])), (out[1], fit[0])
        assert abs(out[2] - fit[1]) <= rel_tol, (out[2], fit[1])
    return 0


@pytest.mark.parametrize("branch", ["std", "small"])
def test_host_entry_equals_the_mirrored_class_on_random_lists(fx, branch):
    pytest.importorskip("sklearn")
    theta, _, rel_tol = fx
    row, zero, vel = K.random_lists(theta, branch)
    out, bits, status, inliers = K.run_host_entry(row, zero, vel, theta)
    F = row.shape[1]
    flagged = sum(_check_against_class(theta, vel, row[0, f], int(zero[0, f]), out[0, f], bits[0, f], status[0, f], inliers[0, f], rel_tol)
                  for f in range(F))
    assert len(set(status.ravel().tolist())) == 3 and flagged * 10 <= F, flagged
    assert np.all((out[0, bits[0] == 0, 0] >= 0.1) == (branch == "std"))


def test_compaction_is_ordered_and_m_cuts_the_rows(fx):
    """Which rows carry the peaks decides which pairs a subset index addresses: moving the peaks to other rows (same columns)
    changes the fit exactly as the class's; rows behind m[f] are absent; m[f] == 0 is an empty list."""
    pytest.importorskip("sklearn")
    theta, cases, rel_tol = fx
    case = next(c for c in cases if c.name == "std_100")
    rng = np.random.default_rng(3)
    rows = [case.row]
    for _ in range(3):
        rows.append(case.row[rng.permutation(case.n_rows)])
    row = np.stack(rows)[None]
    zero = np.full((1, 4), case.zero)
    m = np.array([case.n_rows, case.n_rows, 60, 0], dtype=np.int32)
    zero[0, 2] = zero[0, 3] = -1                                             # no zero-azimuth peak: vx 0.0, the small-vx branch
    out, bits, status, inliers = K.run_host_entry(row, zero, case.vel, theta, m=m)
    for f in range(4):
        assert _check_against_class(theta, case.vel, row[0, f], int(zero[0, f]), out[0, f], bits[0, f], status[0, f], inliers[0, f],
                                    rel_tol, m=int(m[f])) == 0
    assert not np.array_equal(out[0, 0], out[0, 1]) and status[0, 3] == K.EMPTY and out[0, 3, 0] == 0.0 and not np.signbit(out[0, 3, 0])
    # two groups share vx: minus the mean of both zero-azimuth velocities, in NumPy's order
    two = np.stack([case.row, case.row[::-1].copy()])[:, None]
    out, bits, _, _ = K.run_host_entry(two, [[case.zero], [case.zero + 3]], case.vel, theta, g_az=0, g_el=1)
    vx = -1 * (case.vel[case.zero] + case.vel[case.zero + 3]) / 2.0
    assert np.all(bits == 0) and out[0, 0, 0] == vx == out[1, 0, 0]
    only = K.run_host_entry(two, [[case.zero], [case.zero + 3]], case.vel, theta, g_az=0, g_el=1, mode=_lib.DOPAZ_RANSAC_VX_ONLY)
    assert np.all(only[0][..., 0] == vx) and np.all(only[0][..., 1:] == 0.0) and np.all(only[2] == K.OK)


def test_entry_refuses_bad_arguments_and_leaves_outputs_untouched(fx):
    theta, cases, _ = fx
    case = next(c for c in cases if c.name == "std_64")
    row, zero = case.row[None, None], np.array([[case.zero]], dtype=np.int32)
    nan = float("nan")
    bad = [(dict(row_peak=None), "null"), (dict(zero=None), "null"), (dict(vel=None), "null"), (dict(cos=None), "null"),
           (dict(sin=None), "null"), (dict(theta=None), "null"), (dict(subsets=None), "null"), (dict(trials=None), "null"),
           (dict(out=None), "null"), (dict(flags=None), "null"), (dict(G=-1), "negative"), (dict(F=-1), "negative"),
           (dict(n_rows=-1), "negative"), (dict(vel_len=-1), "negative"), (dict(n_tab=-1), "negative"), (dict(trials_len=-1), "negative"),
           (dict(g_az=1), "g_az"), (dict(g_az=-1), "g_az"), (dict(g_el=1), "g_el"), (dict(g_el=-2), "g_el"),
           (dict(vel_len=63), "velocity table"), (dict(n_cols=0), "n_cols"), (dict(n_tab=54), "subset tables"),
           (dict(trials_len=100), "trial table"), (dict(thr_standard=nan), "not finite"), (dict(thr_small_vx=float("inf")), "not finite"),
           (dict(min_R2=nan), "not finite"), (dict(min_inlier_share=nan), "not finite"), (dict(mode=2), "mode"),
           (dict(vel_per_frame=2), "vel_per_frame"), (dict(G=1 << 20, F=1 << 20, g_az=0), "32-bit")]
    for override, text in bad:
        rc, out, flags = K.host_call(row, zero, case.vel, theta, raw=override)
        assert rc == _lib.MMW_ERR_INVALID, override
        assert text in _lib.load_library().mmw_last_error().decode(), (override, _lib.load_library().mmw_last_error())
        assert np.all(out == 7.0) and np.all(flags == -9), override
    for m in ([-1], [65]):
        rc, out, flags = K.host_call(row, zero, case.vel, theta, m=np.array(m, dtype=np.int32))
        assert rc == _lib.MMW_ERR_INVALID and b"m is" in _lib.load_library().mmw_last_error() and np.all(out == 7.0)
    # beyond the rows a wavefront holds: unsupported, and the limit is named
    n = _lib.DOPAZ_RANSAC_MAX_ROWS + 1
    rc, out, _ = K.host_call(np.full((1, 1, 64), -1), zero, case.vel, theta, raw=dict(n_rows=n, vel_len=n, n_tab=n - 9, trials_len=1 << 30))
    assert rc == _lib.MMW_ERR_UNSUPPORTED and b"512" in _lib.load_library().mmw_last_error() and np.all(out == 7.0)
    for override in (dict(F=0), dict(G=0)):                                    # nothing to do: MMW_OK, nothing written
        rc, out, flags = K.host_call(row, zero, case.vel, theta, raw=override)
        assert rc == _lib.MMW_OK and np.all(out == 7.0) and np.all(flags == -9)
    # the device entry judges its arguments before it touches the context: a null context is refused like any null pointer
    lib = _lib.load_library()
    assert lib.mmw_doppler_azimuth_ransac(*([None] * 3 + [1, 1, 64, None, None, 64, 0, None, None, None, 1, None, None, 55, 2000, 0, -1, 0,
                                                          0.15, 0.2, 0.6, 0.75, None, None])) == _lib.MMW_ERR_INVALID


class _Cfg:
    def __init__(self, geometry):
        self.array_geometry, self.virtual_antennas_enabled, self.array_direction, self.range_max_m = geometry, True, "down", 10.0


def _bare_estimator(geometry, **kw):
    from mmwave_radar_processing_amd.processors.velocity_estimator import VelocityEstimator
    est = VelocityEstimator.__new__(VelocityEstimator)
    est.config_manager = _Cfg(geometry)
    est.x_measurement_only = kw.get("x_measurement_only", False)
    est.min_R2_threshold, est.min_inlier_percent = 0.6, 0.75
    est.ego_vx_estimate = -1.0
    est.azimuth_ego_vy_estimate = est.azimuth_estimate_R2 = est.azimuth_inlier_percent = 0.0
    est.elevation_ego_vy_estimate = est.elevation_estimate_R2 = est.elevation_inlier_percent = 0.0
    est.proposed_velocity_estimate = np.empty(shape=0)
    est.current_velocity_estimate = np.array([0.0, 0.0, 0.0])
    return est


def test_state_scan_follows_the_class_frame_by_frame_and_carries_state_across_calls():
    """Tracks written by hand: an empty group keeps its previous fit, a failed fit installs zeros, the proposal is formed in the
    geometry's component order, the gates decide per component, and two calls that split the frames equal one call."""
    ok, empty, failed = K.OK, K.EMPTY, K.FAILED
    fits = np.array([[[1.0, 0.5, 0.9, 0.8], [1.0, -0.2, 0.9, 0.8]],       # both pass
                     [[1.1, 0.6, 0.5, 0.8], [1.1, -0.3, 0.9, 0.7]],       # az fails R^2, el fails the share
                     [[1.2, 0.0, 0.0, 0.0], [1.2, -0.4, 0.9, 0.8]],       # az empty: keeps (0.6, 0.5, 0.8) -> still fails
                     [[1.3, 0.0, 0.0, 0.0], [1.3, 0.0, 0.0, 0.0]],        # az failed: zeros; el empty: keeps frame 2's fit
                     [[1.4, 0.7, 0.6, 0.75], [1.4, -0.5, 0.6, 0.75]]])    # both exactly at the gates: pass
    status = np.array([[ok, ok], [ok, ok], [empty, ok], [failed, empty], [ok, ok]])
    want_ods = np.array([[0.5, -0.2, 1.0], [0.0, 0.0, 1.1], [0.0, -0.4, 1.2], [0.0, -0.4, 1.3], [0.7, -0.5, 1.4]])
    got = dopaz_state_scan(_bare_estimator("ods"), fits, status)
    assert got.shape == (5, 3) and np.array_equal(got, want_ods)
    est = _bare_estimator("ods")
    split = np.concatenate([dopaz_state_scan(est, fits[:3], status[:3]), dopaz_state_scan(est, fits[3:], status[3:])])
    assert np.array_equal(split, want_ods) and est.ego_vx_estimate == 1.4 and est.elevation_inlier_percent == 0.75
    want_std = np.array([[1.0, 0.5, 0.0], [1.1, 0.0, 0.0], [1.2, 0.0, 0.0], [1.3, 0.0, 0.0], [1.4, 0.7, 0.0]])
    assert np.array_equal(dopaz_state_scan(_bare_estimator("standard"), fits[:, :1], status[:, :1]), want_std)
    only_x = dopaz_state_scan(_bare_estimator("standard", x_measurement_only=True), fits[:, :1], status[:, :1])
    assert np.array_equal(only_x[:, 0], fits[:, 0, 0]) and np.all(only_x[:, 1:] == 0.0)
    with pytest.raises(ValueError, match="fits"):
        dopaz_state_scan(_bare_estimator("ods"), fits[:, :1], status)
    with pytest.raises(ValueError, match="groups"):
        dopaz_state_scan(_bare_estimator("ods"), fits[:, :1], status[:, :1])


@pytest.mark.parametrize("name", ["standard", "ods"])
@pytest.mark.parametrize("mode", ["coarse", "precise"])
def test_recorded_reference_tracks_drive_the_state_scan(fx, name, mode):
    """The reference class's recorded per-frame fits through ``dopaz_state_scan``: its recorded current estimates, bit for bit
    (the scan does no arithmetic of its own), whole and split in two calls."""
    track = K.recorded(name, mode)
    status = K.recorded_status(track)
    assert {K.OK, K.EMPTY, K.FAILED} <= set(status.ravel().tolist()) or name == "standard"
    got = dopaz_state_scan(_bare_estimator(name), track["fits"], status)
    assert np.array_equal(got, track["current"])
    est = _bare_estimator(name)
    split = np.concatenate([dopaz_state_scan(est, track["fits"][:6], status[:6]), dopaz_state_scan(est, track["fits"][6:], status[6:])])
    assert np.array_equal(split, track["current"]) and np.array_equal(est.proposed_velocity_estimate, track["proposal"][-1])


def test_plain_fit_prediction_statistics_antenna_sets_and_points_path(fx):
    """The class's methods that need no map: the plain least-squares fit and the prediction against NumPy on a stored list, the
    R^2 statistics of a proposal that is the law itself, the antenna sets of every geometry, and the ``points=`` path, which is
    the two-column fit of the point-cloud estimator behind the standard geometry's gate."""
    pytest.importorskip("sklearn")
    from mmwave_radar_processing_amd.point_cloud_processing.vel_estimator import ransac_fit
    from mmwave_radar_processing_amd.processors import velocity_estimator as ve
    theta, cases, _ = fx
    case = next(c for c in cases if c.name == "std_128")
    rows = np.flatnonzero(case.row >= 0)
    peaks = np.stack([theta[case.row[rows]], case.vel[rows]], axis=1)
    est = _bare_estimator("standard")
    est.valid_angle_bins = theta
    est.ego_vx_estimate = case.vx
    y, H = -1 * peaks[:, 1] - case.vx * np.cos(peaks[:, 0]), np.sin(peaks[:, 0])
    assert est.lsq_fit_ego_vy(peaks) == np.linalg.lstsq(H[:, None], y, rcond=None)[0][0] and est.lsq_fit_ego_vy(peaks[:0]) == 0.0
    v = np.array([1.5, -0.5])
    assert np.abs(est.lsq_predict_velocity_measurement(v) + (np.cos(theta) * 1.5 + np.sin(theta) * -0.5)).max() <= 4 * 2.0 ** -52   # two products, one sum
    on_law = np.stack([theta, est.lsq_predict_velocity_measurement(v)], axis=1)
    est.azimuth_peaks, est.elevation_peaks, est.proposed_velocity_estimate = on_law, np.empty((0, 2)), np.array([1.5, -0.5, 0.0])
    est.compute_R2_statistics()
    assert est.azimuth_estimate_R2 == 1.0
    ods = _bare_estimator("ods")
    ods.valid_angle_bins = theta
    ods.azimuth_peaks = ods.elevation_peaks = on_law
    ods.proposed_velocity_estimate = np.array([-0.5, -0.5, 1.5])
    ods.compute_R2_statistics()
    assert ods.azimuth_estimate_R2 == 1.0 == ods.elevation_estimate_R2
    est.elevation_peaks = on_law
    with pytest.raises(NotImplementedError):
        est.compute_R2_statistics()
    # antenna sets: (geometry, virtual antennas) -> sets, groups, shift_angle
    for geometry, virtual, want in (("standard", True, ([list(range(8))], [(0,)], [True])),
                                    ("standard", False, ([list(range(4))], [(0,)], [True])),
                                    ("ods", True, ([[0, 3, 4, 7], [1, 2, 5, 6], [10, 11, 6, 7], [9, 8, 5, 4]], [(0, 1), (2, 3)], [True, True, False, False])),
                                    ("ods", False, ([[0, 3], [1, 2], [1, 0], [3, 4]], [(0, 1), (2, 3)], [True, True, False, False]))):
        cfg = _Cfg(geometry)
        cfg.virtual_antennas_enabled = virtual
        assert ve.antenna_plan(cfg) == want
    with pytest.raises(ValueError):
        ve.antenna_plan(_Cfg("ring"))
    with pytest.raises(NotImplementedError):
        _bare_estimator("standard").compute_elevation_response(np.zeros((12, 4, 4)), np.array([0.0, 1.0]))
    # points: a clean cloud passes the gate, the ods geometry refuses
    rng = np.random.default_rng(9)
    az = rng.uniform(-1.0, 1.0, 60)
    pts = np.column_stack((3.0 * np.cos(az), 3.0 * np.sin(az), np.zeros(60), -(np.cos(az) * 1.2 + np.sin(az) * -0.4)))
    est = _bare_estimator("standard")
    got = est.process(points=pts)
    coef, r2, share = ransac_fit(pts, 2)
    assert np.array_equal(got, [coef[0], coef[1], 0.0]) and est.azimuth_estimate_R2 == r2 and est.azimuth_inlier_percent == share
    noisy = pts.copy()
    noisy[:, 3] = rng.uniform(-3.0, 3.0, 60)                                    # incoherent speeds: whatever R^2 the inliers give
    got = est.process(points=noisy)
    coef, r2, _ = ransac_fit(noisy, 2)
    assert np.array_equal(got, [coef[0], coef[1], 0.0] if r2 >= est.min_R2_threshold else np.zeros(3))
    est.min_R2_threshold = 2.0                                                  # no fit reaches it: the estimate is zeroed
    assert np.array_equal(est.process(points=pts), np.zeros(3))
    with pytest.raises(NotImplementedError):
        _bare_estimator("ods").process(points=pts)


def test_pipeline_refuses_bad_arguments_before_any_device_use():
    from mmwave_radar_processing_amd import synth
    from mmwave_radar_processing_amd.batch import FramePipeline
    from mmwave_radar_processing_amd.config_managers import ConfigManager
    from mmwave_radar_processing_amd.processors.velocity_estimator import VelocityEstimator, antenna_plan
    cm = ConfigManager()
    cm.load_cfg_text(synth.synth_cfg_text(num_samples=64, num_loops=32))
    est, shape = VelocityEstimator(cm, lower_range_bound=0.5, upper_range_bound=1.5), (12, 64, 32)
    assert antenna_plan(cm) == ([list(range(8))], [(0,)], [True]) and est.ego_vx_estimate == -1.0
    assert np.array_equal(est.get_range_window(altitude=1.0, sensing_direction="down"), [0.5, 2.5])
    p = FramePipeline.__new__(FramePipeline)
    p.n_frames = 3
    p.V, p.S, p.C = shape
    for method in (p.doppler_azimuth_fits, p.doppler_azimuth_velocities):
        with pytest.raises(ValueError, match="VelocityEstimator"):
            method(object(), 1.0)
        with pytest.raises(ValueError, match="altitudes"):
            method(est, [1.0, 2.0])
        with pytest.raises(ValueError, match="altitudes"):
            method(est, [1.0, float("nan"), 2.0])
        est.min_R2_threshold = float("nan")
        with pytest.raises(ValueError, match="gates"):
            method(est, 1.0)
        est.min_R2_threshold = 0.6
    assert not hasattr(p, "ctx") and not hasattr(p, "bufs") and not hasattr(p, "n_dopaz_fits_flagged")


def test_entries_under_address_and_ub_sanitizers(tmp_path):
    """The new translation unit's host code compiled host-only with AddressSanitizer + UndefinedBehaviorSanitizer and linked with
    tests/cpp/doppler_azimuth_velocity_sanitize.cpp, a program of its own that launches nothing: the refusals with the outputs
    left untouched, F == 0 and G == 0, through both entries, and the shared rule on the boundary sizes through the host-only
    one.  (No GPU sanitizer is involved; the kernel is a launch stub that is never reached.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-ffp-contract=off", "--cuda-host-only"]
    obj = str(tmp_path / "mmw_tu_dopaz_velocity.o")
    subprocess.run([hipcc, *flags, "-c", "-o", obj, os.path.join(csrc, "mmw_tu_dopaz_velocity.hip")], check=True)
    # the host-only object still refers to its (absent) device code object: an empty stand-in, never launched
    nm = shutil.which("nm") or "/usr/bin/nm"
    undefined = subprocess.run([nm, "-u", obj], capture_output=True, text=True, check=True).stdout
    fatbins = sorted({ln.split()[-1] for ln in undefined.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "fatbin_stubs.cpp"
    stub.write_text("".join(f'extern "C" const char {name}[16] __attribute__((aligned(4096))) = {{0}};\n' for name in fatbins))
    exe = str(tmp_path / "doppler_azimuth_velocity_sanitize")
    subprocess.run([hipcc, *flags, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "doppler_azimuth_velocity_sanitize.cpp"), "-x", "c++",
                    str(stub), "-x", "none", obj, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
