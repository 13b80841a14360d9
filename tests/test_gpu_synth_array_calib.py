"""mmw_synth_array_calibrate on the device.  The reference-generated fixture (cases a, b, c) through
``FramePipeline.synthetic_array_calibrated``: targets and status equal the reference's, no frame flagged, responses within the
project's spectra bar of each response's peak, geometry within ``SPEC_TOL lambda / 2 pi`` (a geometry error must not be able to
consume the spectra bar by itself).  The entry itself on hazard shapes against the host functions of the class (float64 numpy
contraction): S = 63 and 64, E = 102 with a chirp stride, the 16-byte path, H = 1, windows longer than the buffer, two elevation
bins, enough frames for the tiled GEMM path.  The same kinds of shape through the pipeline, naturally flagged and with every frame
flagged: each flagged frame bit-equal to the host functions on its downloaded window.  The host route under ``MMW_SYNTH_CALIB_FLAG_ALL``; a decoy antenna and poisoned
outputs; the uncalibrated path bit-identical before and after."""
import ctypes

import numpy as np
import pytest

from mmwave_radar_processing_amd import _lib, synth
from mmwave_radar_processing_amd.batch import FramePipeline
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.processors import SyntheticArrayBeamformerProcessor
from mmwave_radar_processing_amd.processors import synthetic_array_beamformer as sab
from test_synth_array_calib_host import LAMBDA, case_processor, directions, numpy_contract

pytestmark = pytest.mark.gpu

SPEC_TOL = 1e-5
POISON64 = np.frombuffer(np.array([0x7FC00ABC, 0x7FC00DEF], dtype=np.uint32).tobytes(), dtype=np.complex64)[0]


def virtual_cubes(g):
    n, _, S, L = g["slabs"].shape
    virt = np.zeros((n, 12, S, L), dtype=np.complex64)
    virt[:, [int(a) for a in g["live"]]] = g["slabs"]
    return virt


@pytest.fixture(scope="module")
def fixture_pipeline(golden):
    g = golden("synth_array_calib.npz")
    proc = case_processor(g, "a", cls=SyntheticArrayBeamformerProcessor)
    fp = FramePipeline(proc.config_manager, max_frames=8, shape=(12, 63, 100))
    fp.load(virtual_cubes(g))
    return g, fp


@pytest.mark.parametrize("flag_all", [0, 1])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_fixture_cases_through_the_pipeline(fixture_pipeline, case, flag_all):
    g, fp = fixture_pipeline
    proc = case_processor(g, case, cls=SyntheticArrayBeamformerProcessor)
    before = fp.synthetic_array(proc, g["velocities"])[1]
    fp.ctx.set_option("MMW_SYNTH_CALIB_FLAG_ALL", flag_all or None)
    try:
        frames, resp = fp.synthetic_array_calibrated(proc, g["velocities"], num_calibration_iters=int(g[f"{case}_iters"]))
    finally:
        fp.ctx.set_option("MMW_SYNTH_CALIB_FLAG_ALL", None)
    assert frames.tolist() == g[f"{case}_frames"].tolist() and resp.shape == g[f"{case}_responses"].shape
    assert fp.n_flagged == (3 if flag_all else 0)           # zero flagged frames is a condition: the fixture's margins are asserted
    assert np.array_equal(fp.synth_calib_targets, g[f"{case}_targets"]) and np.array_equal(fp.synth_calib_status, g[f"{case}_status"])
    want_P = g[f"{case}_geometry_calibrated"].transpose(0, 2, 1, 3).reshape(3, 3, -1)
    geo = 2 * np.pi * np.abs(fp.synth_geometry_calibrated - want_P).max() / float(g["lambda_m"])
    worst = max(np.abs(resp[i] - g[f"{case}_responses"][i]).max() / g[f"{case}_peaks"][i] for i in range(3))
    print(f"case {case} flag_all {flag_all}: geometry 2 pi |dP| / lambda {geo:.3g}, responses {worst:.3g} of the peak")
    assert geo <= SPEC_TOL and worst <= SPEC_TOL
    # the uncalibrated path on the same frames, before and after: bit-identical
    assert np.array_equal(fp.synthetic_array(proc, g["velocities"])[1].view(np.float64), before.view(np.float64))


# ------------------------------------------------------------------------------------------------------------------ hazard shapes
def hazard_scene(n, S, C, k, d, seed):
    """Cubes [n, 2, S, C] (antenna 1: three reflectors along a perturbed track; antenna 0: a decoy with other reflectors) over noise of sigma 6, integer
    valued -- a column whose samples sum to exactly zero at row 0 or S / 2 sends its frames to the host, about one frame in 200 here --
    and the nominal absolute element positions [n, 3, Cv] the geometry tables are cut from."""
    rng = np.random.default_rng(seed)
    Cv, n_az = len(range(0, C, k)), d.shape[1]
    t = np.arange(n * C).reshape(n, C)
    nominal = np.zeros((n, 3, C))
    nominal[:, 0] = 4e-4 * t + 2e-3 * np.arange(n)[:, None]         # a gap between frames
    true = nominal.copy()
    true[:, 0] *= 1.004
    true[:, 1] = 1e-6 * t
    rows = rng.choice(np.arange(3, S - 3, 4), 3, replace=False)
    azs = rng.choice(np.arange(1, n_az - 1), 3, replace=False)
    s = np.arange(S)[:, None]
    x = 6.0 * (rng.standard_normal((n, 2, S, C)) + 1j * rng.standard_normal((n, 2, S, C)))
    for f in range(n):
        for q, (r, a) in enumerate(zip(rows, azs)):
            x[f, 1] += (90 - 15 * q) * np.exp(2j * np.pi * r * s / S) * np.exp(-2j * np.pi * (d[:, a, 0] @ true[f]) / LAMBDA)[None, :]
            x[f, 0] += 120 * np.exp(2j * np.pi * ((r + 2) % S) * s / S) * np.exp(-2j * np.pi * (d[:, (a + 1) % n_az, 0] @ nominal[f]) / LAMBDA)[None, :]
    cubes = (np.round(x.real) + 1j * np.round(x.imag)).astype(np.complex64)
    return cubes, nominal[:, :, ::k], Cv


def window_of(cubes, nominal, k, H, frame):
    S, Cv = cubes.shape[2], nominal.shape[2]
    X = np.concatenate([cubes[fr, 1][:, ::k] if fr >= 0 else np.zeros((S, Cv), np.complex64) for fr in range(frame - H + 1, frame + 1)], axis=1)
    P = np.concatenate([nominal[fr] if fr >= 0 else nominal[0] - 1.0 for fr in range(frame - H + 1, frame + 1)], axis=1)
    return X.astype(complex), P


HAZARDS = {
    # n_resident, S, C, k, H, n_az, n_el, n_iters
    "S=63 E=102 stride 3": (10, 63, 100, 3, 3, 13, 2, 1),
    "S=64 E=32 16-byte path": (10, 64, 16, 1, 2, 9, 1, 2),
    "H=1": (10, 64, 40, 1, 1, 9, 1, 1),
    "H longer than the buffer": (3, 32, 16, 1, 4, 7, 1, 1),
    "600 frames (tiled GEMM)": (600, 64, 16, 1, 2, 9, 1, 1),
}


@pytest.mark.parametrize("name", list(HAZARDS))
def test_hazard_shapes_against_the_host_functions(name):
    n, S, C, k, H, n_az, n_el, n_it = HAZARDS[name]
    d = directions(n_az, n_el)
    cubes, nominal, Cv = hazard_scene(n, S, C, k, d, seed=len(name))
    E, T = H * Cv, n_az * n_el
    frames = np.arange(n, dtype=np.int32)
    win = [window_of(cubes, nominal, k, H, f) for f in frames]
    P = np.ascontiguousarray(np.stack([w[1] for w in win]))
    ctx = _lib.default_context()
    d_cubes = ctx.alloc(cubes.nbytes)
    d_cubes.upload(cubes)
    guard = 64
    d_out, d_P, d_st, d_tg = ctx.alloc((n * S * T + guard) * 8), ctx.alloc((n * 3 * E + guard) * 8), ctx.alloc(n * 4), ctx.alloc(n * 24)
    d_out.upload(np.full(n * S * T + guard, POISON64, dtype=np.complex64))
    d_P.upload(np.full(n * 3 * E + guard, -7.0))
    dirs = np.ascontiguousarray(d.reshape(3, -1))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)

    def call(**over):
        a = dict(v=1, n_iters=n_it, n_az=n_az, lam=LAMBDA)
        a.update(over)
        return ctx.lib.mmw_synth_array_calibrate(ctx.handle, d_cubes.ptr, n, 2, S, C, a["v"], k, H, frames.ctypes.data_as(ip), n,
                                                 P.ctypes.data_as(dp), dirs.ctypes.data_as(dp), a["n_az"], n_el, a["lam"], a["n_iters"],
                                                 d_out.ptr, d_P.ptr, d_st.ptr, d_tg.ptr)
    try:
        # refusals write nothing
        for over in (dict(v=2), dict(n_iters=0), dict(n_iters=9), dict(n_az=0), dict(lam=0.0)):
            assert call(**over) == _lib.MMW_ERR_INVALID
        assert np.isnan(d_out.download((n * S * T + guard,), np.complex64)).all() and (d_P.download((n * 3 * E + guard,), np.float64) == -7.0).all()
        _lib.check(call())
        out = d_out.download((n * S * T + guard,), np.complex64)
        Pcal = d_P.download((n * 3 * E + guard,), np.float64)
        assert np.isnan(out[n * S * T:]).all() and (Pcal[n * 3 * E:] == -7.0).all(), "guard overwritten"
        out, Pcal = out[:n * S * T].reshape(n, S, n_az, n_el), Pcal[:n * 3 * E].reshape(n, 3, E)
        assert not np.isnan(out).any()
        status, targets = d_st.download((n,), np.int32), d_tg.download((n, 3, 2), np.int32)
    finally:
        for b in (d_cubes, d_out, d_P, d_st, d_tg):
            b.free()
    flagged = np.flatnonzero(status < 0)
    print(f"{name}: {len(flagged)} of {n} frames flagged, status counts {np.unique(status, return_counts=True)}")
    assert len(flagged) * 10 <= n
    worst_g = worst_r = 0.0
    step = max(1, n // 40)          # (the long batch: every 15th frame against the host, all of them for status)
    for i in range(0, n, step):
        X, Pi = win[i]
        if status[i] < 0:      # the raw entry hands such a frame back untouched (whatever iteration flagged it); the host route
            assert np.array_equal(Pcal[i], Pi) and (targets[i] == -1).all()      # is test_hazard_shapes_through_the_pipeline's
            continue
        contract = lambda g: numpy_contract(X, g, d, LAMBDA)      # noqa: E731
        resp, want_P, want_t, want_s = sab.calibrate_window(X, Pi, d, LAMBDA, n_it, contract(Pi), contract)
        tg = np.full((3, 2), -1)
        tg[:len(want_t)] = np.array(want_t).reshape(-1, 2)
        assert status[i] == want_s and np.array_equal(targets[i], tg), (i, status[i], want_s, targets[i], want_t)
        worst_g = max(worst_g, 2 * np.pi * np.abs(Pcal[i] - want_P).max() / LAMBDA)
        worst_r = max(worst_r, np.abs(out[i] - resp).max() / np.abs(resp).max())
    if H > n:
        assert (status == 0).all() and np.array_equal(Pcal, P)      # a slot before the buffer: no suitable targets
    else:
        assert (status[H - 1:][status[H - 1:] >= 0] == n_it).all() and (status[:H - 1] == 0).all()
    print(f"{name}: geometry 2 pi |dP| / lambda {worst_g:.3g}, responses {worst_r:.3g} of the peak")
    assert worst_g <= SPEC_TOL and worst_r <= SPEC_TOL


# ------------------------------------------------------------------------------------------- hazard shapes through the pipeline
PIPELINE_HAZARDS = {
    # frames, S, loops, stride, H, n_az, n_el, n_iters
    "stride 1, H=1, one elevation": (12, 64, 40, 1, 1, 9, 1, 1),
    "16-byte path, two iterations": (12, 64, 16, 1, 2, 9, 1, 2),
    "stride 3, H=3, two elevations": (10, 63, 100, 3, 3, 13, 2, 1),
    "600 frames": (600, 64, 16, 1, 2, 9, 1, 1),
}
PIPE_VEL = np.array([4.0, 0.2, 0.0])           # 0.4 wavelengths between chirps of one transmitter, frames back to back


def pipeline_scene(name):
    """A configuration whose frames follow each other without a gap, a plain processor on receiver 1 / transmitter 2, and virtual
    cubes [n, 12, S, loops]: antenna 9 sees three reflectors along a track 0.4 % longer than the reported one (noise sigma 6,
    integer valued), the other antennas a decoy."""
    n, S, L, k, H, n_az, n_el, n_it = PIPELINE_HAZARDS[name]
    period_ms = np.ceil(3 * L * 67e-3 * 10 + 1) / 10
    cm = ConfigManager()
    cm.load_cfg_text(synth.synth_cfg_text(num_samples=S, num_loops=L).replace(f" {L} 0 100 1 0", f" {L} 0 {period_ms:g} 1 0"))
    proc = SyntheticArrayBeamformerProcessor(cm, receiver_idx=1, chirp_cfg_idx=2, num_frames=H, stride=k,
                                             az_angle_bins_rad=np.deg2rad(np.linspace(5, 65, n_az)),
                                             el_angle_bins_rad=np.deg2rad(np.linspace(0, 10, n_el)), min_vel=np.zeros(3),
                                             max_vel=np.full(3, 10.0), max_vel_stdev=np.full(3, 10.0))
    assert proc.frame_period_ms == period_ms
    rng = np.random.default_rng(len(name))
    idx = 3 * np.arange(L) + 2                                            # raw chirp of loop c of transmitter 2
    t_s = -(3 * L - 1 - idx) * proc.chirp_period_us * 1e-6
    rows = rng.choice(np.arange(3, S - 3, 4), 3, replace=False)
    azs = rng.choice(np.arange(1, n_az - 1), 3, replace=False)
    s = np.arange(S)[:, None]
    x = 6.0 * (rng.standard_normal((n, 12, S, L)) + 1j * rng.standard_normal((n, 12, S, L)))
    for f in range(n):
        pos = (2 * PIPE_VEL * period_ms * 1e-3 * f)[:, None] + 2 * t_s[None, :] * PIPE_VEL[:, None]
        pos[0] *= 1.004
        for q, (r, a) in enumerate(zip(rows, azs)):
            x[f, 9] += (90 - 15 * q) * np.exp(2j * np.pi * r * s / S) * np.exp(-2j * np.pi * (proc.d[:, a, 0] @ pos) / proc.lambda_m)[None, :]
            x[f, 5] += 120 * np.exp(2j * np.pi * ((r + 2) % S) * s / S)
    return proc, (np.round(x.real) + 1j * np.round(x.imag)).astype(np.complex64), n_it


@pytest.mark.parametrize("name", list(PIPELINE_HAZARDS))
def test_hazard_shapes_through_the_pipeline(name):
    n, S, L, k, H, n_az, n_el, n_it = PIPELINE_HAZARDS[name]
    proc, cubes, n_it = pipeline_scene(name)
    vel = np.tile(PIPE_VEL, (n, 1))
    fp = FramePipeline(proc.config_manager, max_frames=n, shape=(12, S, L))
    fp.load(cubes)
    runs = {}
    try:
        for flag_all in (0, 1):
            fp.ctx.set_option("MMW_SYNTH_CALIB_FLAG_ALL", flag_all or None)
            try:
                frames, resp = fp.synthetic_array_calibrated(proc, vel, num_calibration_iters=n_it)
            finally:
                fp.ctx.set_option("MMW_SYNTH_CALIB_FLAG_ALL", None)
            runs[flag_all] = (frames, resp, fp.synth_geometry_calibrated.copy(), fp.synth_calib_status.copy(), fp.synth_calib_targets.copy(),
                              fp.n_flagged)
        # which frames the device flagged of its own accord: the raw entry on the same arguments
        v, fr32, P, dirs, _, _ = fp._synthetic_array_arguments(proc, vel, "test")
        E, T = P.shape[2], n_az * n_el
        d_P, d_st, d_tg = fp.ctx.alloc(len(fr32) * 3 * E * 8), fp.ctx.alloc(len(fr32) * 4), fp.ctx.alloc(len(fr32) * 24)
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        _lib.check(fp.ctx.lib.mmw_synth_array_calibrate(fp.ctx.handle, fp.d_in.ptr, n, 12, S, L, v, k, H, fr32.ctypes.data_as(ip), len(fr32),
                                                        P.ctypes.data_as(dp), dirs.ctypes.data_as(dp), n_az, n_el, float(proc.lambda_m), n_it,
                                                        fp.d_synth.ptr, d_P.ptr, d_st.ptr, d_tg.ptr))
        raw_status = d_st.download((len(fr32),), np.int32)
        for b in (d_P, d_st, d_tg):
            b.free()
        # the windows as the host route sees them: downloaded from the resident cubes
        slab = S * L * 8
        got_cubes = np.stack([fp.d_in.download((S, L), np.complex64, byte_offset=(f * 12 + v) * slab) for f in range(n)])
    finally:
        fp.bufs.free()
    assert np.array_equal(got_cubes, cubes[:, 9])
    frames = runs[0][0]
    assert frames.tolist() == list(range(H - 1, n)) and np.array_equal(runs[1][0], frames)
    natural = np.flatnonzero(raw_status < 0)
    assert runs[0][5] == len(natural) and runs[1][5] == len(frames)
    print(f"{name}: {len(natural)} of {len(frames)} frames flagged by the device; status counts {np.unique(runs[0][3], return_counts=True)}")
    d, lam = proc.d, float(proc.lambda_m)
    worst_g = worst_r = 0.0
    exact = 0
    for i, f in enumerate(frames):
        X = np.concatenate([cubes[fr, 9][:, ::k] for fr in range(f - H + 1, f + 1)], axis=1).astype(complex)
        contract = lambda g: numpy_contract(X, g, d, lam)         # noqa: E731
        resp, want_P, want_t, want_s = sab.calibrate_window(X, P[i], d, lam, n_it, contract(P[i]), contract)
        tg = np.full((3, 2), -1)
        tg[:len(want_t)] = np.array(want_t).reshape(-1, 2)
        for flag_all in (0, 1):
            _, got, Pcal, status, targets, _ = runs[flag_all]
            assert status[i] == want_s and np.array_equal(targets[i], tg), (flag_all, i, status[i], want_s, targets[i].tolist(), want_t)
            if flag_all or raw_status[i] < 0:       # the host route: the same functions on the same window, bit for bit
                assert np.array_equal(Pcal[i], want_P), (flag_all, i)
                exact += 1
            worst_g = max(worst_g, 2 * np.pi * np.abs(Pcal[i] - want_P).max() / lam)
            worst_r = max(worst_r, np.abs(got[i] - resp).max() / np.abs(resp).max())
    print(f"{name}: {exact} host-route results bit-equal; geometry 2 pi |dP| / lambda {worst_g:.3g}, responses {worst_r:.3g} of the peak")
    assert exact >= len(frames) and worst_g <= SPEC_TOL and worst_r <= SPEC_TOL
    assert (runs[0][3] == n_it).any()               # the scene calibrates: the comparison is not one of empty results
