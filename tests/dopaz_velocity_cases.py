"""Shared cases of the Doppler-azimuth RANSAC tests (host and GPU): the stored fixture (tests/golden/dopaz_velocity.npz, written by
make_golden_dopaz_velocity.py from the reference class), callers of the two C entries, and lists built to sit on a decision."""
import ctypes as C
import os

import numpy as np

from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.point_cloud_processing import ransac_tables as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dopaz_velocity.npz")
THR = (0.15, 0.20)
MIN_R2, MIN_SHARE = 0.6, 0.75
OK, EMPTY, FAILED = _lib.DOPAZ_STATUS_OK, _lib.DOPAZ_STATUS_EMPTY, _lib.DOPAZ_STATUS_FAILED
_fixture = None
_tracks = {}


class Case:
    def __init__(self, name, n_rows, vel, row, zero, clear, ref):
        self.name, self.n_rows, self.vel, self.row, self.zero, self.clear = name, int(n_rows), vel, row, int(zero), bool(clear)
        self.vx, self.vy, self.r2, self.share = (float(x) for x in ref[:4])
        self.inliers, self.status = int(ref[4]), int(ref[5])


def fixture():
    """(theta, cases, rel_tol); installs the recorded subset and trial tables, so no scikit-learn is needed afterwards."""
    global _fixture
    if _fixture is None:
        z = np.load(GOLDEN)
        subsets, trials = z["table_subsets"].astype(np.int32), z["table_trials"].astype(np.int32)
        off = 0
        for i, n in enumerate(range(T.MIN_SAMPLES, T.MIN_SAMPLES + len(subsets))):
            T.seed_tables(n, subsets[i], trials[off:off + n + 1])
            off += n + 1
        cases, o = [], 0
        for i, name in enumerate(z["case_names"]):
            n = int(z["case_n_rows"][i])
            cases.append(Case(str(name), n, z["case_vel"][o:o + n].copy(), z["case_row"][o:o + n].astype(np.int32), z["case_zero"][i],
                              z["case_clear"][i], z["case_ref"][i]))
            o += n
        _fixture = (z["theta"].copy(), cases, float(z["rel_tol"]))
        for name in ("standard", "ods"):
            for mode in ("coarse", "precise"):
                _tracks[(name, mode)] = {k: z[f"seq_{name}_{mode}_{k}"] for k in ("fits", "counts", "proposal", "current")}
    return _fixture


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def decode(flags):
    flags = np.asarray(flags)
    return (flags & _lib.DOPAZ_FLAG_MASK, (flags >> _lib.DOPAZ_STATUS_SHIFT) & _lib.DOPAZ_STATUS_MASK, flags >> _lib.DOPAZ_INLIERS_SHIFT)


def tables_for(n_rows, cos=None, sin=None, theta=None):
    subsets, trials = T.dopaz_tables(n_rows)
    return subsets, trials, max(n_rows - T.MIN_SAMPLES + 1, 0)


def host_call(row_peak, zero, vel, theta, m=None, cos=None, sin=None, g_az=0, g_el=-1, mode=0, thr=THR, min_r2=MIN_R2,
              min_share=MIN_SHARE, out=None, flags=None, raw=None):
    """``mmw_diag_doppler_azimuth_ransac_host`` -> (status code, out, flags); ``raw`` replaces raw arguments by name."""
    row_peak = np.ascontiguousarray(row_peak, dtype=np.int32)
    zero = np.ascontiguousarray(zero, dtype=np.int32)
    G, F, n_rows = row_peak.shape
    vel = np.ascontiguousarray(vel, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    cos = np.cos(theta) if cos is None else np.ascontiguousarray(cos, dtype=np.float64)
    sin = np.sin(theta) if sin is None else np.ascontiguousarray(sin, dtype=np.float64)
    subsets, trials, n_tab = tables_for(n_rows)
    out = np.full((G, F, 4), 7.0) if out is None else out
    flags = np.full((G, F), -9, dtype=np.int32) if flags is None else flags
    h_m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
    a = dict(row_peak=_p(row_peak), zero=_p(zero), G=G, F=F, n_rows=n_rows, h_m=None if h_m is None else h_m.ctypes.data_as(_lib._ip),
             vel=_p(vel), vel_len=vel.shape[-1], vel_per_frame=int(vel.ndim == 2), cos=_p(cos), sin=_p(sin), theta=_p(theta),
             n_cols=len(theta), subsets=_p(subsets), trials=_p(trials), n_tab=n_tab, trials_len=len(trials), g_az=g_az, g_el=g_el,
             mode=mode, thr_standard=thr[0], thr_small_vx=thr[1], min_R2=min_r2, min_inlier_share=min_share, out=_p(out),
             flags=_p(flags))
    a.update(raw or {})
    rc = _lib.load_library().mmw_diag_doppler_azimuth_ransac_host(*a.values())
    return rc, out, flags


def run_host_entry(row_peak, zero, vel, theta, **kw):
    rc, out, flags = host_call(row_peak, zero, vel, theta, **kw)
    _lib.check(rc)
    return (out,) + decode(flags)


def run_device_entry(ctx, row_peak, zero, vel, theta, m=None, g_az=0, g_el=-1, mode=0, thr=THR, min_r2=MIN_R2, min_share=MIN_SHARE):
    """``mmw_doppler_azimuth_ransac`` on uploaded copies -> (out, raw flags)."""
    row_peak = np.ascontiguousarray(row_peak, dtype=np.int32)
    zero = np.ascontiguousarray(zero, dtype=np.int32)
    G, F, n_rows = row_peak.shape
    vel = np.ascontiguousarray(vel, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    subsets, trials, n_tab = tables_for(n_rows)
    host = [row_peak, zero, vel, np.cos(theta), np.sin(theta), theta, subsets, trials]
    dev = []
    for arr in host:
        d = ctx.alloc(max(arr.nbytes, 8))
        d.upload(np.ascontiguousarray(arr))
        dev.append(d)
    d_out, d_flags = ctx.alloc(G * F * 32), ctx.alloc(G * F * 4)
    d_out.upload(np.full((G, F, 4), 7.0))
    d_flags.upload(np.full((G, F), -9, dtype=np.int32))
    h_m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
    try:
        _lib.check(ctx.lib.mmw_doppler_azimuth_ransac(
            ctx.handle, dev[0].ptr, dev[1].ptr, G, F, n_rows, None if h_m is None else h_m.ctypes.data_as(_lib._ip), dev[2].ptr,
            vel.shape[-1], int(vel.ndim == 2), dev[3].ptr, dev[4].ptr, dev[5].ptr, len(theta), dev[6].ptr, dev[7].ptr, n_tab,
            len(trials), g_az, g_el, mode, thr[0], thr[1], min_r2, min_share, d_out.ptr, d_flags.ptr))
        return d_out.download((G, F, 4), np.float64).copy(), d_flags.download((G, F), np.int32).copy()
    finally:
        for d in dev + [d_out, d_flags]:
            d.free()


def check_against_reference(case, out, bits, status, inliers, rel_tol):
    """The assertions of one (unflagged or flagged) pair against the recorded reference values."""
    if bits:
        assert np.all(out == 0.0) and status == OK and inliers == 0, case.name
        return
    assert out[0] == case.vx and np.signbit(out[0]) == np.signbit(case.vx), (case.name, out[0], case.vx)
    assert status == case.status, (case.name, status, case.status)
    if case.status != OK:
        assert np.all(out[1:] == 0.0), case.name
        return
    assert inliers == case.inliers and out[3] == case.share, (case.name, inliers, out[3])
    assert abs(out[1] - case.vy) <= rel_tol * max(1.0, abs(case.vy)), (case.name, out[1], case.vy)
    assert abs(out[2] - case.r2) <= rel_tol, (case.name, out[2], case.r2)


def batches(cases, theta, per_frame_tables):
    """The crafted lists as launches (n_rows, row_peak [1, F, n_rows], zero [1, F], vel, cases): all lists of one n_rows in one
    launch with a velocity table per frame, or one launch per list with its table shared."""
    for n_rows in sorted({c.n_rows for c in cases}):
        group = [c for c in cases if c.n_rows == n_rows]
        if per_frame_tables:
            yield n_rows, np.stack([c.row for c in group])[None], np.array([[c.zero for c in group]]), np.stack([c.vel for c in group]), group
        else:
            for c in group:
                yield n_rows, c.row[None, None], np.array([[c.zero]]), c.vel, [c]


def residual_at_threshold(theta):
    """A standard-branch list with one peak whose residual is the threshold itself: at theta = 0 (H = 0) the residual is |y| =
    |-v - vx| whatever the fit, and v is chosen 0.15 below -vx."""
    n_rows = 64
    vel = np.arange(n_rows) * (4.0 / n_rows) - 2.0
    zero = int(np.argmin(np.abs(vel + 0.5)))
    vx = -1 * vel[zero]
    rng = np.random.default_rng(5)
    row = np.full(n_rows, -1, dtype=np.int32)
    for r in rng.permutation(n_rows)[:40]:
        row[r] = int(np.argmin(np.abs(-(vx * np.cos(theta) - 0.6 * np.sin(theta)) - vel[r])))
    vel = vel.copy()
    r0 = int(np.flatnonzero(row < 0)[0])
    row[r0] = int(np.argmin(np.abs(theta)))
    vel[r0] = -(vx + 0.15)
    assert theta[row[r0]] == 0.0 and abs(abs(-1 * vel[r0] - vx) - 0.15) < 1e-15
    return row, zero, vel


def mirrored_trials(theta, n=64):
    """A small-vx list whose second trial is the mirror image of its first: an involution of the rows that maps the first subset
    onto the second, paired rows sharing their velocity and carrying opposite angles (rows of both subsets: angle 0).  The two
    fits are c and -c, the inlier sets mirror images of equal size, the scores equal up to rounding: a tie between different
    sets.  The velocity table repeats entries, which the entry allows."""
    sub = T.subset_table(n)
    s0, s1 = [int(i) for i in sub[0]], [int(i) for i in sub[1]]
    both = [i for i in s0 if i in s1]
    only0, only1 = [i for i in s0 if i not in s1], [i for i in s1 if i not in s0]
    rest = [i for i in range(n) if i not in s0 and i not in s1]
    pairs = list(zip(only0, only1)) + list(zip(rest[0::2], rest[1::2]))
    fixed = both + (rest[-1:] if len(rest) % 2 else [])
    rng = np.random.default_rng(17)
    centre = int(np.argmin(np.abs(theta)))
    assert theta[centre] == 0.0 and np.array_equal(theta, -theta[::-1])
    vel = np.zeros(n)
    row = np.full(n, centre, dtype=np.int32)
    for a, b in pairs:
        h = rng.uniform(0.3, 1.5) * rng.choice([-1.0, 1.0])
        col = int(np.argmin(np.abs(theta - 0.8 * h))) if rng.random() < 0.5 else int(rng.integers(0, len(theta)))
        vel[a] = vel[b] = h
        row[a], row[b] = col, len(theta) - 1 - col
    for i in fixed:
        vel[i] = rng.uniform(-1.5, 1.5)
    zero = n                       # an extra row holds vx = 0
    return np.r_[row, -1].astype(np.int32), zero, np.r_[vel, 0.0]


def random_lists(theta, branch, count=200, n_rows=128, seed=1):
    """``count`` random peak lists of one regression branch ("std" / "small") as one launch: (row_peak [1, count, n_rows],
    zero [1, count], vel).  0 .. 99 peaks each, three in four near the cosine law of a random (vx, vy), the rest anywhere."""
    rng = np.random.default_rng(seed + (0 if branch == "std" else 1000))
    vel = np.linspace(-3.0, 3.0, n_rows, endpoint=False)
    cos, sin = np.cos(theta), np.sin(theta)
    row = np.full((1, count, n_rows), -1, dtype=np.int32)
    zero = np.full((1, count), -1, dtype=np.int32)
    for f in range(count):
        vx_want = rng.uniform(0.2, 2.5) if branch == "std" else rng.uniform(-0.3, 0.09)
        zero[0, f] = int(np.argmin(np.abs(vel + vx_want)))
        vx = -1 * vel[zero[0, f]]
        vy = rng.uniform(0.3, 1.5) * rng.choice([-1.0, 1.0])
        n, used = int(rng.integers(0, 100)), set()
        for _ in range(2 * n):
            c = int(rng.integers(0, len(theta)))
            r = int(rng.integers(0, n_rows)) if rng.random() < 0.25 else int(np.argmin(np.abs(vel + (vx * cos[c] + vy * sin[c]))))
            if r not in used and len(used) < n:
                used.add(r)
                row[0, f, r] = c
    return row, zero, vel


# ------------------------------------------------------------------------------------------------ the recorded sequences
ESTIMATOR_KW = dict(lower_range_bound=0.5, upper_range_bound=1.5)


def sequence_cfg(name):
    """(cfg text, ConfigManager keyword arguments, cube shape, frames) of a recorded sequence."""
    import json
    from mmwave_radar_processing_amd import synth
    if name == "standard":
        return synth.synth_cfg_text(num_samples=256, num_loops=128), {}, (12, 256, 128), 16
    with open(os.path.join(os.path.dirname(GOLDEN), "cfg_scalars.json")) as f:
        return "\n".join(json.load(f)["6843_RadVel_ods_20Hz.cfg"]["lines"]), {"array_geometry": "ods"}, (12, 63, 70), 24


def sequence(name, range_res_m, vel_res_m_s):
    """(cubes [F, 12, S, C], altitudes [F]) of a recorded sequence, made from its seed: a platform that starts almost at rest
    (the small-vx branch) and speeds up, movers in some frames (the gates), one lost frame (empty groups)."""
    from mmwave_radar_processing_amd import synth
    _, _, shape, F = sequence_cfg(name)
    f = np.arange(F)
    vel = np.stack([0.3 + 1.6 * f, -12.0 + 1.0 * f], axis=1) * vel_res_m_s        # in velocity bins: every size sees rows of peaks
    movers = np.where(f % 5 == 3, 30, np.where(f % 5 == 1, 12, 0))
    cubes, _ = synth.synth_moving_platform_sequence(2025 + len(name), F, shape, range_res_m, vel_res_m_s, name, (1.1, 2.9), vel,
                                                    num_scatterers=96, movers=movers, dropouts=(6,))
    return cubes, 1.4 + 0.2 * f / F


def recorded(name, mode):
    """The reference class's ``process`` over a sequence, per frame: ``fits [F, G, 4]`` (vx, vy, R^2, share as the class held them
    after the frame), ``counts [F, G]`` (row peaks of the frame; 0: the fit kept the previous values), ``proposal [F, 3]`` and
    ``current [F, 3]``."""
    fixture()
    return _tracks[(name, mode)]


def recorded_status(track):
    """The status table the recorded frames imply: no row peaks EMPTY; fewer than 10, or a fit that came back as three zeros,
    FAILED (the scan installs zeros for it either way)."""
    fits, counts = track["fits"], track["counts"]
    failed = (counts < 10) | np.all(fits[..., 1:] == 0.0, axis=2)
    return np.where(counts == 0, EMPTY, np.where(failed, FAILED, OK)).astype(np.int32)
