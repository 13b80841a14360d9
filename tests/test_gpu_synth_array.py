"""mmw_synth_array on the device: the windowed operand of the Bartlett contraction read in place from resident cubes, through
every kernel path, against the float64 restatement ``oracle.bartlett_response`` on the host-stacked window (zeros for frames
before the buffer).  The bar is the project's spectra bar: every value within 1e-5 of that response's peak.  Every frame and
antenna of a scene carries its own tone and amplitude, so a wrong slab, a window off by a frame or a chirp off by one shows at the
order of the peak.  The output buffer is poisoned and has guard elements behind it."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.processors import SyntheticArrayBeamformerProcessor
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

SPEC_TOL = 1e-5
LAMBDA = 299792458.0 / 60.25e9
POISON = np.frombuffer(np.array([0x7FC00ABC, 0x7FC00DEF], dtype=np.uint32).tobytes(), dtype=np.complex64)[0]
GUARD = 64
N_RES = 6
# context options that force each kernel: the steering-fused tile kernels and the tiled GEMM behind k_steer
PATHS = {
    "tile32 f32": {"MMW_BARTLETT_PATH": 1, "MMW_BARTLETT_TILE16": 0, "MMW_BARTLETT_BF16": 0},
    "tile32 bf16x3": {"MMW_BARTLETT_PATH": 1, "MMW_BARTLETT_TILE16": 0},
    "tile32 poly": {"MMW_BARTLETT_PATH": 1, "MMW_BARTLETT_POLY": 1},
    "tile16": {"MMW_BARTLETT_PATH": 1, "MMW_BARTLETT_TILE16": 1},
    "gemm bf16x3": {"MMW_BARTLETT_PATH": 2},
    "gemm f32": {"MMW_BARTLETT_PATH": 2, "MMW_BARTLETT_BF16": 0},
    "default": {},
}


def scene(n, V, S, C, seed):
    """Integer-valued cubes [n, V, S, C]: frame f, antenna a carries the tone (row 1 + 2 f + a, Doppler bin 1 + a + 3 f) with
    amplitude 40 + 9 f + 23 a, plus noise of sigma 2."""
    rng = np.random.default_rng(seed)
    s, c = np.arange(S)[:, None], np.arange(C)[None, :]
    x = 2.0 * (rng.standard_normal((n, V, S, C)) + 1j * rng.standard_normal((n, V, S, C)))
    for f in range(n):
        for a in range(V):
            x[f, a] += (40 + 9 * f + 23 * a) * np.exp(2j * np.pi * ((1 + 2 * f + a + 0.3) * s / S + (1 + a + 3 * f + 0.2) * c / C))
    return (np.round(x.real) + 1j * np.round(x.imag)).astype(np.complex64)


def stacked_window(cubes, v, k, H, frame):
    """X [S, E]: the window of `frame`, oldest first, zeros for frames before the buffer."""
    S = cubes.shape[2]
    parts = [cubes[fr, v][:, ::k] if fr >= 0 else np.zeros((S, len(range(0, cubes.shape[3], k))), np.complex64)
             for fr in range(frame - H + 1, frame + 1)]
    return np.concatenate(parts, axis=1)


def directions(T):
    naz, nel = {14: (7, 2), 33: (11, 3), 7: (7, 1), 32: (32, 1), 4: (2, 2)}[T]
    return O.steering_dirs(np.linspace(-0.9, 0.9, naz), np.linspace(-0.3, 0.3, nel) if nel > 1 else np.array([0.0]))


class Device:
    """Resident cubes + a poisoned output buffer with guard elements behind it."""

    def __init__(self, cubes, n_out_max, T):
        self.ctx = _lib.default_context()
        self.cubes = cubes
        self.n, self.V, self.S, self.C = cubes.shape
        self.d_cubes = self.ctx.alloc(cubes.nbytes)
        self.d_cubes.upload(cubes)
        self.cap = n_out_max * self.S * T + GUARD
        self.d_out = self.ctx.alloc(self.cap * 8)

    def poison(self):
        self.d_out.upload(np.full(self.cap, POISON, dtype=np.complex64))

    def raw(self):
        return self.d_out.download((self.cap,), np.complex64)

    def call(self, v, k, H, frames, P, dirs, lam=LAMBDA, over=None):
        frames = np.ascontiguousarray(frames, dtype=np.int32)
        P = np.ascontiguousarray(P, dtype=np.float64)
        dirs = np.ascontiguousarray(np.asarray(dirs, dtype=np.float64).reshape(3, -1))
        dp = ctypes.POINTER(ctypes.c_double)
        a = dict(ctx=self.ctx.handle, d_cubes=self.d_cubes.ptr, n=self.n, V=self.V, S=self.S, C=self.C, v=v, k=k, H=H,
                 frames=frames.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n_out=len(frames), P=P.ctypes.data_as(dp),
                 dirs=dirs.ctypes.data_as(dp), T=dirs.shape[1], lam=lam, out=self.d_out.ptr)
        a.update(over or {})
        return self.ctx.lib.mmw_synth_array(a["ctx"], a["d_cubes"], a["n"], a["V"], a["S"], a["C"], a["v"], a["k"], a["H"], a["frames"],
                                            a["n_out"], a["P"], a["dirs"], a["T"], a["lam"], a["out"])

    def run(self, v, k, H, frames, P, dirs):
        """Poison, call, check the guard and that every output was written; [n_out, S, T] complex64."""
        self.poison()
        _lib.check(self.call(v, k, H, frames, P, dirs))
        raw = self.raw()
        n = len(frames) * self.S * np.asarray(dirs).reshape(3, -1).shape[1]
        assert np.array_equal(raw[n:].view(np.uint32), np.full(self.cap - n, POISON).astype(np.complex64).view(np.uint32)), "guard overwritten"
        assert not np.isnan(raw[:n]).any(), "an output element was not written"
        return raw[:n].reshape(len(frames), self.S, -1)

    def free(self):
        self.d_cubes.free()
        self.d_out.free()


def check_paths(dev, v, k, H, frames, T, paths, seed):
    """One reference per call shape, every path against it; the worst ratio to the bar's peak."""
    Cv = len(range(0, dev.C, k))
    rng = np.random.default_rng(seed)
    P = rng.uniform(-0.05, 0.05, (len(frames), 3, H * Cv))
    d = directions(T)
    refs = [O.bartlett_response(stacked_window(dev.cubes, v, k, H, fr).astype(complex), P[i], d, LAMBDA).reshape(dev.S, T)
            for i, fr in enumerate(frames)]
    worst = {}
    for name in paths:
        for key, val in PATHS[name].items():
            dev.ctx.set_option(key, val)
        try:
            out = dev.run(v, k, H, frames, P, d)
        finally:
            for key in PATHS[name]:
                dev.ctx.set_option(key, None)
        worst[name] = max(float(np.abs(out[i] - refs[i]).max() / np.abs(refs[i]).max()) for i in range(len(frames)))
    return worst


SHAPES = {
    "E=32 over four frames": (2, 16, 8, 1, 4, 14),
    "chunks straddle, second column tile partly filled": (2, 40, 20, 1, 3, 33),
    "odd C, Tp padding": (2, 63, 21, 1, 2, 14),
    "strided, Cv=7": (3, 33, 20, 3, 3, 7),
    "fully aligned fast case": (2, 32, 32, 1, 2, 32),
    "one chirp": (2, 8, 1, 1, 2, 4),
    "one sample": (2, 1, 8, 1, 2, 4),
    "K split (E = 256)": (2, 16, 64, 1, 4, 14),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_path_at_every_hazard_shape(name):
    V, S, C, k, H, T = SHAPES[name]
    dev = Device(scene(N_RES, V, S, C, seed=S * 100 + C), 4, T)
    try:
        for v in (0, V - 1):
            for frames in ([0, 1, 4, 5], [5]):      # windows that reach before the buffer, a gap; then one output alone
                worst = check_paths(dev, v, k, H, frames, T, list(PATHS), seed=v + len(frames))
                print(f"{name} v={v} frames={frames}: " + ", ".join(f"{p} {w:.2e}" for p, w in worst.items()))
                assert max(worst.values()) <= SPEC_TOL, worst
    finally:
        dev.free()


@pytest.mark.parametrize("H", [1, 8])
def test_window_of_one_frame_and_window_longer_than_the_buffer(H):
    V, S, C, T = 2, 40, 20, 14
    dev = Device(scene(N_RES, V, S, C, seed=H), N_RES, T)
    try:
        worst = check_paths(dev, 1, 1, H, list(range(N_RES)), T, list(PATHS), seed=H)
        print(f"H={H}: " + ", ".join(f"{p} {w:.2e}" for p, w in worst.items()))
        assert max(worst.values()) <= SPEC_TOL, worst
    finally:
        dev.free()


def test_markers_tell_slab_frame_and_chirp_apart():
    """The reference itself moves at the order of the peak when the window is taken from the wrong antenna, one frame late or one
    chirp late: what the bar of the other tests would catch."""
    V, S, C, k, H = 3, 33, 20, 3, 3
    cubes = scene(N_RES, V, S, C, seed=5)
    d = directions(7)
    P = np.random.default_rng(1).uniform(-0.05, 0.05, (3, H * 7))
    good = O.bartlett_response(stacked_window(cubes, 1, k, H, 4).astype(complex), P, d, LAMBDA)
    peak = np.abs(good).max()
    shifted = np.roll(cubes, -1, axis=3)
    for wrong in (stacked_window(cubes, 2, k, H, 4), stacked_window(cubes, 1, k, H, 3), stacked_window(shifted, 1, k, H, 4)):
        assert np.abs(O.bartlett_response(wrong.astype(complex), P, d, LAMBDA) - good).max() > 0.05 * peak


def test_bad_arguments_leave_the_output_poisoned_and_a_good_call_follows():
    V, S, C, k, H, T = 2, 16, 8, 1, 2, 4
    dev = Device(scene(N_RES, V, S, C, seed=9), 2, T)
    try:
        P = np.random.default_rng(2).uniform(-0.05, 0.05, (2, 3, H * C))
        d = directions(T)
        dev.poison()
        bad = [dict(ctx=None), dict(d_cubes=None), dict(frames=None), dict(P=None), dict(dirs=None), dict(out=None),
               dict(v=-1), dict(v=V), dict(k=0), dict(k=-3), dict(H=0), dict(H=-1), dict(T=0), dict(T=-2), dict(lam=0.0),
               dict(lam=-LAMBDA)]
        for over in bad:
            assert dev.call(0, k, H, [1, 4], P, d, over=over) == _lib.MMW_ERR_INVALID, over
            assert dev.ctx.lib.mmw_last_error(), over
        for frames in ([4, 1], [3, 3], [1, N_RES], [-1, 2]):        # unsorted, repeated, out of range
            assert dev.call(0, k, H, frames, P, d) == _lib.MMW_ERR_INVALID, frames
        with pytest.raises(ValueError, match="ascending"):
            _lib.check(dev.call(0, k, H, [3, 3], P, d))
        # no outputs: OK, nothing written
        assert dev.call(0, k, H, [], P, d) == _lib.MMW_OK
        dev.ctx.sync()
        assert np.array_equal(dev.raw().view(np.uint32), np.full(dev.cap, POISON).astype(np.complex64).view(np.uint32))
        # a good call afterwards on the same buffers
        out = dev.run(1, k, H, [1, 4], P, d)
        for i, fr in enumerate([1, 4]):
            ref = O.bartlett_response(stacked_window(dev.cubes, 1, k, H, fr).astype(complex), P[i], d, LAMBDA).reshape(S, T)
            assert np.abs(out[i] - ref).max() <= SPEC_TOL * np.abs(ref).max()
    finally:
        dev.free()


def test_profile_family_is_registered():
    V, S, C, k, H, T = 2, 16, 8, 1, 2, 4
    dev = Device(scene(N_RES, V, S, C, seed=9), 2, T)
    try:
        P = np.zeros((2, 3, H * C))
        dev.ctx.profile_enable(True)
        dev.ctx.profile_reset()
        try:
            _lib.check(dev.call(0, k, H, [1, 4], P, directions(T)))
            dev.ctx.sync()
            ms, n = dev.ctx.profile_get("synth_array")
        finally:
            dev.ctx.profile_enable(False)
        assert n == 1 and ms > 0
    finally:
        dev.free()


# ---------------------------------------------------------------- the reference-generated fixture
def fixture_setup(g):
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as fh:
        lines = json.load(fh)[str(g["cfg"])]["lines"]
    cm = ConfigManager()
    cm.load_cfg_text("\n".join(lines) + "\n")
    rx, cfg_idx, H, stride = (int(x) for x in g["params"])
    proc = SyntheticArrayBeamformerProcessor(cm, receiver_idx=rx, chirp_cfg_idx=cfg_idx, num_frames=H, stride=stride,
                                             az_angle_bins_rad=g["az_rad"], el_angle_bins_rad=g["el_rad"], min_vel=g["min_vel"],
                                             max_vel=g["max_vel"], max_vel_stdev=g["max_vel_stdev"])
    n, _, S, L = g["slabs"].shape
    virt = np.zeros((n, 12, S, L), dtype=np.complex64)
    virt[:, g["live"]] = g["slabs"]
    raw = np.zeros((n, 4, S, 3 * L), dtype=np.complex64)
    for tx in range(3):
        raw[:, :, :, tx::3] = virt[:, 4 * tx:4 * tx + 4]
    return cm, proc, virt, raw


def worst_ratio(got, g):
    return max(float(np.abs(got[i] - g["responses"][i]).max() / g["peaks"][i]) for i in range(len(g["peaks"])))


def test_fixture_class_stepped_over_the_raw_cubes(golden):
    g = golden("synth_array.npz")
    _, proc, _, raw = fixture_setup(g)
    got = []
    for f, vel in enumerate(g["velocities"]):
        out = proc.process(raw[f], vel)
        assert (out.size > 0) == bool(g["valid"][f])
        if out.size:
            assert out.shape == (63, 7, 2) and out.dtype == np.complex128 and out is proc.beamformed_resp
            got.append(out)
    worst = worst_ratio(got, g)
    print(f"class, stepped: worst deviation {worst:.2e} of the peak")
    assert worst <= SPEC_TOL


def test_fixture_pipeline_after_load_and_load_raw(golden):
    g = golden("synth_array.npz")
    cm, proc, virt, raw = fixture_setup(g)
    state = (proc.history_avg_vel.copy(), proc.history_acd_cube_valid_chirps.copy(), proc.array_geometry_valid)
    fp = FramePipeline(cm, max_frames=8, shape=(12, 63, 100))
    results = []
    for how in ("load", "load_raw"):
        fp.load(virt) if how == "load" else fp.load_raw(raw, num_tx=3)
        frames, resp = fp.synthetic_array(proc, g["velocities"])
        assert frames.tolist() == [2, 3, 7] and resp.shape == (3, 63, 7, 2) and resp.dtype == np.complex128
        worst = worst_ratio(resp, g)
        print(f"pipeline after {how}: worst deviation {worst:.2e} of the peak")
        assert worst <= SPEC_TOL
        results.append(resp)
    assert np.array_equal(results[0], results[1])
    # the device form: the same bits, nothing downloaded by the call
    frames, d = fp.synthetic_array_device(proc, g["velocities"])
    dev = d.download((3, 63, 14), np.complex64)
    assert frames.tolist() == [2, 3, 7] and np.array_equal(dev.astype(np.complex128).reshape(3, 63, 7, 2), results[1])
    assert np.array_equal(proc.history_avg_vel, state[0]) and np.array_equal(proc.history_acd_cube_valid_chirps, state[1])
    assert proc.array_geometry_valid is state[2]
    # no frame valid: empty results, no launch
    frames, resp = fp.synthetic_array(proc, np.zeros((8, 3)))
    assert frames.shape == (0,) and resp.shape == (0, 63, 7, 2)
