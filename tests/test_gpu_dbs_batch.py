"""Batched Doppler beam sharpening (FramePipeline.dbs_range_angle, mmw_dbs_sharpen) against the float64 oracle, the per-frame
processor, the committed golden frame and single-bin NumPy DFTs.

Error measure of a sharpened frame: max|got - want| / max|fft3d_windowed(cube[rx], A)| <= SPEC_TOL -- the picked columns need
not hold the frame's peak, and the float32 range-Doppler error scales with the plane's peak.  Slow frames (plain range-angle):
rel_err as the range-angle tests have it.  Measured maxima are printed by every parity test."""
import ctypes
import functools

import numpy as np
import pytest

from mmwave_radar_processing_amd import _lib, synth
from mmwave_radar_processing_amd.batch import FramePipeline
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.processors import RangeAngleProcessorDBSEnhanced
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu
SPEC_TOL = 1e-5
# (V, S, C), A, n_out, F: the fused 256 x 128 range-Doppler kernel; a shipped non-power-of-two plane; more frames than one wave
# of workgroups on the smallest plane
CASES = {"fused": ((12, 256, 128), 64, 64, 3), "mixed": ((12, 63, 100), 64, 64, 3), "tiny": ((4, 8, 16), 8, 5, 70)}
RX_LISTS = {"all": (), "four": (0, 1, 2, 3), "two": (1, 3)}


def rel_err(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@functools.lru_cache(maxsize=None)
def setup(case):
    (V, S, C), A, n_out, F = CASES[case]
    cm = ConfigManager()
    cm.load_cfg_text(synth.synth_cfg_text(num_samples=S, num_loops=C))
    dbs = RangeAngleProcessorDBSEnhanced(cm, num_angle_bins_range_angle_response=A, num_angle_bins_dbs_enhanced_response=n_out)
    assert len(dbs.vel_bins) == C
    cubes = np.stack([synth.synth_cube(900 + 7 * f, (V, S, C)) for f in range(F)])
    cubes.setflags(write=False)
    return cm, dbs, cubes


def velocities(cm, F, slow, seed=0):
    """A different velocity per frame, up to 0.8 vel_max in the plane; the frames in ``slow`` move below min_vel_dbs."""
    rng = np.random.default_rng(seed)
    phi = rng.uniform(0, 2 * np.pi, F)
    speed = rng.uniform(0.3, 0.8, F) * cm.vel_max_m_s
    v = np.stack([speed * np.cos(phi), speed * np.sin(phi), rng.normal(size=F)], axis=1)
    for f in slow:
        v[f] = [0.1, -0.05, 2.0]
    return v


@functools.lru_cache(maxsize=None)
def oracle_cube(case, rx):
    """|fft3d_windowed(cube[rx], A)| of every frame of the case (float64) and its peaks."""
    _, dbs, cubes = setup(case)
    mags = [np.abs(O.fft3d_windowed(c[list(rx)] if rx else c, dbs.num_angle_bins)) for c in cubes]
    return mags, [float(m.max()) for m in mags]


def oracle_frames(case, rx, v, chirp_idx=0):
    _, dbs, cubes = setup(case)
    mags, peaks = oracle_cube(case, rx)
    out = []
    for f in range(len(cubes)):
        if np.linalg.norm(v[f][0:2]) < dbs.min_vel_dbs:
            out.append(O.range_angle(cubes[f], dbs.num_angle_bins, chirp_idx, rx))
        else:
            out.append(O.dbs_sharpen(mags[f], v[f], dbs.angle_bins_no_dbs_enhancement, dbs.angle_bins_dbs_enhanced, dbs.vel_bins))
    return out, peaks


def pipeline(case, load=True):
    cm, dbs, cubes = setup(case)
    p = FramePipeline(cm, max_frames=len(cubes), shape=cubes.shape[1:], num_angle_bins=dbs.num_angle_bins)
    if load:
        p.load(cubes)
    return p


def check_frames(got, want, peaks, sharp, label):
    worst_fast = worst_slow = 0.0
    for f, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == np.float64, (label, f)
        if sharp[f]:
            worst_fast = max(worst_fast, float(np.max(np.abs(g - w))) / peaks[f])
        else:
            worst_slow = max(worst_slow, rel_err(g, w))
    print(f"{label}: sharpened max|got-want|/peak {worst_fast:.3e}, slow rel_err {worst_slow:.3e}")
    assert worst_fast <= SPEC_TOL and worst_slow <= SPEC_TOL
    return worst_fast


SLOW_SETS = [("fused", "mid", (1,)), ("fused", "end", (2,)), ("mixed", "mid", (1,)), ("mixed", "end", (2,)),
             ("tiny", "both", (35, 69))]


@pytest.mark.parametrize("case,where,slow", SLOW_SETS)
def test_matches_the_oracle_per_frame(case, where, slow):
    cm, dbs, cubes = setup(case)
    (V, S, C), A, n_out, F = CASES[case]
    v = velocities(cm, F, slow)
    p = pipeline(case)
    got = p.dbs_range_angle(dbs, v, chirp_idx=1)
    want, peaks = oracle_frames(case, (), v, chirp_idx=1)
    assert len(got) == F and p.dbs_sharpened.tolist() == [f not in slow for f in range(F)]
    assert all(got[f].shape == ((S, A) if f in slow else (S, n_out)) for f in range(F))
    check_frames(got, want, peaks, p.dbs_sharpened, f"oracle {case}/{where}")


@pytest.mark.parametrize("case", ["fused", "mixed", "tiny"])
@pytest.mark.parametrize("rx_name", ["four", "two"])
def test_antenna_lists(case, rx_name):
    """A subset is Hann-windowed over the subset; np.hanning(2) is [0, 0], so two antennas give exactly zero."""
    cm, dbs, cubes = setup(case)
    F = len(cubes)
    rx = RX_LISTS[rx_name]
    v = velocities(cm, F, (F - 1,), seed=1)
    p = pipeline(case)
    got = p.dbs_range_angle(dbs, v, rx_antennas=list(rx))
    want, peaks = oracle_frames(case, rx, v)
    if rx_name == "two":
        for f in np.flatnonzero(p.dbs_sharpened):
            assert not np.any(got[f]) and not np.any(want[f])
        peaks = [1.0] * F                   # the all-zero window: every cube is zero, and so must every difference be
    check_frames(got, want, peaks, p.dbs_sharpened, f"rx {rx_name} {case}")


@pytest.mark.parametrize("case", ["fused", "mixed", "tiny"])
def test_agrees_with_the_per_frame_processor(case):
    """Entry f has the values of ``dbs.process(cube_f, ...)`` within SPEC_TOL of the frame's peak (slow frames: of their own)."""
    cm, dbs, cubes = setup(case)
    F = len(cubes)
    rx = (0, 1, 2, 3)
    frames = list(range(F)) if F <= 3 else [0, 34, 35, 36, 68, 69]
    v = velocities(cm, F, (F // 2,), seed=2)
    p = pipeline(case)
    got = p.dbs_range_angle(dbs, v, rx_antennas=np.array(rx), chirp_idx=2)
    _, peaks = oracle_cube(case, rx)
    worst = 0.0
    for f in frames:
        one = dbs.process(cubes[f], velocity_ned=v[f], rx_antennas=np.array(rx), chirp_idx=2)
        assert one.shape == got[f].shape
        scale = peaks[f] if p.dbs_sharpened[f] else float(np.max(np.abs(one)))
        worst = max(worst, float(np.max(np.abs(one - got[f]))) / scale)
    print(f"per-frame loop {case}: max difference / peak {worst:.3e}")
    assert worst <= SPEC_TOL


def test_golden_frame_as_a_batch_of_one(golden):
    g = golden("small_chain.npz")
    cm = ConfigManager()
    cm.load_cfg_text(synth.synth_cfg_text(num_samples=32, num_loops=16))
    cube = synth.synth_cube(101, (12, 32, 16))
    dbs = RangeAngleProcessorDBSEnhanced(cm, num_angle_bins_range_angle_response=64, num_angle_bins_dbs_enhanced_response=40)
    p = FramePipeline(cm, max_frames=1, shape=(12, 32, 16))
    p.load(cube[None])
    out = p.dbs_range_angle(dbs, np.asarray(g["p2_dbs_vel"]).reshape(1, 3))
    assert len(out) == 1 and out[0].shape == g["p2_dbs"].shape and p.dbs_sharpened.tolist() == [True]
    print(f"golden: rel_err {rel_err(out[0], g['p2_dbs']):.3e}")
    assert rel_err(out[0], g["p2_dbs"]) <= SPEC_TOL
    slow = p.dbs_range_angle(dbs, np.zeros((1, 3)), chirp_idx=2)
    assert p.dbs_sharpened.tolist() == [False] and rel_err(slow[0], g["p2_ra_all"]) <= SPEC_TOL


def ip(a):
    return a.ctypes.data_as(_lib._ip)


def test_abi_with_hand_built_tables():
    """Angle index 0 and A - 1 and Doppler index 0 and C - 1 in one frame, against single-bin DFTs of the oracle's range-Doppler
    cube; the frames before and after the call's keep their sentinel; d_rd, when given, keeps the range-Doppler cubes."""
    cm, dbs, cubes = setup("mixed")
    (V, S, C), A, _, F = CASES["mixed"]
    ctx = _lib.default_context()
    ang = np.array([[0, A - 1, 0, A - 1, A // 2, 7], [A - 1, A - 1, 0, 0, 1, A // 2 - 1]], dtype=np.int32)
    vel = np.array([[0, C - 1, C - 1, 0, C // 2, 3], [0, 0, C - 1, C - 1, 2, C // 2 + 1]], dtype=np.int32)
    n_out = ang.shape[1]
    d_in, d_rd, d_out = ctx.alloc(cubes.nbytes), ctx.alloc(2 * V * S * C * 8), ctx.alloc(4 * S * n_out * 4)
    try:
        d_in.upload(cubes)
        d_out.upload(np.full((4, S, n_out), -7.0, dtype=np.float32))
        rx, n_rx = _lib.int_array([])
        # frames 1 and 2 of the batch into output slots 1 and 2
        _lib.check(ctx.lib.mmw_dbs_sharpen(ctx.handle, d_in.at(V * S * C * 8), d_rd.ptr, ip(ang), ip(vel), d_out.at(S * n_out * 4),
                                           2, V, S, C, A, rx, n_rx, n_out))
        got = d_out.download((4, S, n_out), np.float32)
        rd_got = d_rd.download((2, V, S, C), np.complex64)
        assert np.all(got[0] == -7.0) and np.all(got[3] == -7.0)
        w = np.hanning(V)
        worst = 0.0
        for f in range(2):
            rd = O.range_doppler(cubes[1 + f])
            assert rel_err(rd_got[f], rd) <= SPEC_TOL
            peak = float(np.max(np.abs(O.fft3d_windowed(cubes[1 + f], A))))
            for i in range(n_out):
                b = (int(ang[f, i]) - A // 2) % A
                want = np.abs(np.einsum("j,js->s", w * np.exp(-2j * np.pi * np.arange(V) * b / A), rd[:, :, vel[f, i]]))
                worst = max(worst, float(np.max(np.abs(got[1 + f][:, i] - want))) / peak)
        print(f"hand-built tables: max|got-want|/peak {worst:.3e}")
        assert worst <= SPEC_TOL
        # nothing to do: MMW_OK without a launch (and without looking at the pointers)
        assert ctx.lib.mmw_dbs_sharpen(ctx.handle, None, None, None, None, None, 0, V, S, C, A, rx, 0, n_out) == _lib.MMW_OK
        assert ctx.lib.mmw_dbs_sharpen(ctx.handle, None, None, None, None, None, 2, V, S, C, A, rx, 0, 0) == _lib.MMW_OK
    finally:
        for b in (d_in, d_rd, d_out):
            b.free()


def test_abi_refuses_bad_tables_and_launches_nothing():
    cm, dbs, cubes = setup("tiny")
    (V, S, C), A, n_out, _ = CASES["tiny"]
    F = 3
    ctx = _lib.default_context()
    lib = ctx.lib
    d_in, d_out = ctx.alloc(F * V * S * C * 8), ctx.alloc(F * S * n_out * 4)
    try:
        d_in.upload(cubes[:F])
        d_out.upload(np.full((F, S, n_out), -7.0, dtype=np.float32))
        ang = np.tile(np.arange(n_out, dtype=np.int32), (F, 1))
        vel = np.tile(np.arange(n_out, dtype=np.int32) * 3, (F, 1))
        no_rx, _ = _lib.int_array([])

        def call(a, k, rx=no_rx, n_rx=0, A_=A):
            return lib.mmw_dbs_sharpen(ctx.handle, d_in.ptr, None, ip(a), ip(k), d_out.ptr, F, V, S, C, A_, rx, n_rx, n_out)

        def message():
            return lib.mmw_last_error().decode()

        for bad, tab, what in ((A, "ang", "angle"), (-1, "ang", "angle"), (C, "vel", "Doppler"), (-1, "vel", "Doppler")):
            a, k = ang.copy(), vel.copy()
            (a if tab == "ang" else k)[1, 2] = bad
            assert call(a, k) == _lib.MMW_ERR_INVALID
            assert "frame 1, entry 2" in message() and what in message() and str(bad) in message()
        for bad in (V, -1):
            rx, n_rx = _lib.int_array([0, bad, 2])
            assert call(ang, vel, rx, n_rx) == _lib.MMW_ERR_INVALID
            assert "rx entry 1" in message() and str(bad) in message()
        assert call(ang, vel, A_=V - 1) == _lib.MMW_ERR_INVALID and "angle bins" in message()        # A < n
        ctx.sync()
        assert np.all(d_out.download((F, S, n_out), np.float32) == -7.0)
        assert call(ang, vel) == _lib.MMW_OK                                                        # the same call, valid
        assert not np.any(d_out.download((F, S, n_out), np.float32) == -7.0)
    finally:
        d_in.free()
        d_out.free()


def test_device_buffer_leaves_slow_frames_unwritten_and_the_cubes_alone():
    cm, dbs, cubes = setup("tiny")
    (V, S, C), A, n_out, F = CASES["tiny"]
    slow = (0, 35, 69)
    v = velocities(cm, F, slow, seed=3)
    p = pipeline("tiny")
    before = p.cubes()
    d = p.dbs_range_angle_device(dbs, v)                # allocates the buffer
    d.upload(np.full((F, S, n_out), -7.0, dtype=np.float32))
    assert p.dbs_range_angle_device(dbs, v) is d
    got = d.download((F, S, n_out), np.float32)
    want, peaks = oracle_frames("tiny", (), v)
    for f in range(F):
        if f in slow:
            assert np.all(got[f] == -7.0) and not p.dbs_sharpened[f]
        else:
            assert p.dbs_sharpened[f] and float(np.max(np.abs(got[f] - want[f]))) / peaks[f] <= SPEC_TOL
    host = p.dbs_range_angle(dbs, v)
    for f in np.flatnonzero(p.dbs_sharpened):
        np.testing.assert_array_equal(host[f], got[f].astype(np.float64))
    after = p.cubes()
    assert before.tobytes() == after.tobytes() == cubes.tobytes()


@pytest.mark.parametrize("case", ["fused", "tiny"])
def test_a_second_call_gives_the_second_answer(case):
    cm, dbs, cubes = setup(case)
    F = len(cubes)
    p = pipeline(case)
    v1, v2 = velocities(cm, F, (), seed=4), velocities(cm, F, (1,), seed=5)
    first = p.dbs_range_angle(dbs, v1)
    second = p.dbs_range_angle(dbs, v2)
    want1, peaks = oracle_frames(case, (), v1)
    want2, _ = oracle_frames(case, (), v2)
    check_frames(first, want1, peaks, [True] * F, f"first call {case}")
    check_frames(second, want2, peaks, p.dbs_sharpened, f"second call {case}")
    assert any(not np.array_equal(a, b) for a, b in zip(first, second))


def test_every_way_of_loading_the_frames():
    """synth(), load_raw(), load_raw_i16() and a stream() chunk hold the frames the method works on."""
    cm, dbs, cubes = setup("tiny")
    (V, S, C), A, n_out, F = CASES["tiny"]
    v = velocities(cm, F, (10,), seed=6)
    want, peaks = oracle_frames("tiny", (), v)
    p = pipeline("tiny", load=False)
    halves = [(0, 35), (35, 70)]
    it = iter(halves)

    def work(pipe):
        lo, hi = next(it)
        return pipe.dbs_range_angle(dbs, v[lo:hi]), pipe.dbs_sharpened.copy()
    got, sharp = [], []
    for frames, flags in p.stream([cubes[lo:hi] for lo, hi in halves], work=work):
        got += frames
        sharp += flags.tolist()
    check_frames(got, want, peaks, sharp, "stream chunks")
    # integer-valued raw cubes: complex64 and int16 I/Q hold the same samples
    num_tx = 2
    raw = np.stack([c.reshape(num_tx, V // num_tx, S, C).transpose(1, 2, 3, 0).reshape(V // num_tx, S, C * num_tx) for c in cubes[:4]])
    p.load_raw(raw, num_tx)
    virt = p.cubes()
    a = p.dbs_range_angle(dbs, v[:4])
    p.load_raw_i16(np.stack([raw.real, raw.imag], axis=-1).astype(np.int16), num_tx)
    assert np.array_equal(p.cubes(), virt)
    b = p.dbs_range_angle(dbs, v[:4])
    p.load(virt)
    c = p.dbs_range_angle(dbs, v[:4])
    for f in range(4):
        np.testing.assert_array_equal(a[f], c[f])
        np.testing.assert_array_equal(b[f], c[f])
        want_f = O.dbs_sharpen(np.abs(O.fft3d_windowed(virt[f], A)), v[f], dbs.angle_bins_no_dbs_enhancement,
                               dbs.angle_bins_dbs_enhanced, dbs.vel_bins)
        assert float(np.max(np.abs(c[f] - want_f))) / float(np.max(np.abs(O.fft3d_windowed(virt[f], A)))) <= SPEC_TOL
    p.synth(5, seed0=77)
    s = p.cubes()
    d = p.dbs_range_angle(dbs, v[:5])
    for f in range(5):
        mag = np.abs(O.fft3d_windowed(s[f], A))
        want_f = O.dbs_sharpen(mag, v[f], dbs.angle_bins_no_dbs_enhancement, dbs.angle_bins_dbs_enhanced, dbs.vel_bins)
        assert float(np.max(np.abs(d[f] - want_f))) / float(mag.max()) <= SPEC_TOL
