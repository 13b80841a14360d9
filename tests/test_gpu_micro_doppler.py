"""Batched micro-Doppler rows (mmw_micro_doppler, MicroDopplerProcessor, FramePipeline.micro_doppler) on the device.

Expected values: ``np.abs(np.fft.fftshift(np.fft.fft2(x[rx]), axes=1))[lo:hi + 1].max(0)`` in float64 on the complex64 cube, and
the reference-generated fixture.  Bar (the project's spectra bar): every value within 1e-5 x the largest magnitude of that
frame's full plane for that antenna.  Every parity test prints the worst ratio it saw.

Shapes: the smallest at which a path of the kernel can go wrong.  3x64x32 power of two; 4x63x20 odd S, composite C; 2x40x23
prime C (every C takes the same direct sums; there is no separate awkward-length path); 2x16x1 and 2x1x8 degenerate axes;
12x63x100 from the fixture (more than 64 chirps: both columns of a lane live).  The kernel dispatches on the number of window rows
K (4, 8 or 16 rows in flight: K <= 4, K <= 8, beyond; more than 16 rows take several passes, the last one partly filled) -- the
windows below hit each -- and loops over blocks of 128 chirps: 2x8x130 is the smallest shape with a second block."""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline, micro_doppler_history
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.processors import MicroDopplerProcessor

pytestmark = pytest.mark.gpu
SPEC_TOL = 1e-5
POISON = np.float32(-7.0)               # no result is negative
GUARD = 64
SHAPES = [(3, 64, 32), (4, 63, 20), (2, 40, 23), (2, 16, 1), (2, 1, 8), (2, 8, 130)]


class GridConfig:
    """The five scalars the processor and the pipeline read: S range bins at 0, 1, ... metres, C velocity bins 1 m/s apart."""

    def __init__(self, S, C):
        self.range_res_m, self.range_max_m = 1.0, float(S)
        self.vel_res_m_s, self.vel_max_m_s = 1.0, C / 2
        self.frameCfg_periodicity_ms = 50.0


def windows(S):
    """(lo, hi): a single row, lo == 0, hi == S - 1, the full span -- K = 1 / up to 8 / more than 8 / S rows."""
    out = {(S // 2, S // 2), (0, min(5, S - 1)), (max(0, S - 20), S - 1), (0, S - 1)}
    if S > 20:
        out.add((S // 3, S // 3 + 2))       # an inner window of 3 rows with all four marker tones
    return sorted(out)


def tone_cubes(shape, lo, hi, F=2, seed=0):
    """On-bin complex tones at the range rows lo - 1, lo, hi, hi + 1 (where they exist), each at its own Doppler bin and amplitude,
    the strongest at lo; every antenna with other Doppler bins and amplitudes; low noise.  A window off by a row, a shift off by
    a bin or a wrong slab then shows as an error of the order of the peak."""
    V, S, C = shape
    rng = np.random.default_rng([seed, S, C, lo, hi])
    s, c = np.arange(S)[:, None], np.arange(C)[None, :]
    cubes = np.zeros((F, V, S, C), dtype=np.complex128)
    for f in range(F):
        for v in range(V):
            x = 0.02 * (rng.standard_normal((S, C)) + 1j * rng.standard_normal((S, C)))
            for i, (row, amp) in enumerate(((lo - 1, 3.0), (lo, 4.0), (hi, 2.0), (hi + 1, 2.5))):
                if 0 <= row < S:
                    dop = (1 + 5 * i + 2 * v + f) % C
                    x = x + (amp + 0.3 * v) * np.exp(2j * np.pi * (row * s / S + dop * c / C))
            cubes[f, v] = x
    return cubes.astype(np.complex64)


def expected(cube, rx, lo, hi):
    """(row, peak of the full plane) of one frame, float64, as the reference computes it."""
    plane = np.abs(np.fft.fftshift(np.fft.fft2(cube[rx]), axes=1))
    return plane[lo:hi + 1].max(0), float(plane.max())


def run_abi(ctx, cubes, rx, lo, hi, n_frames=None, first=0):
    """mmw_micro_doppler on frames [first, first + n_frames) of ``cubes`` into a poisoned buffer with guard elements behind it:
    (status, the whole buffer)."""
    F, V, S, C = cubes.shape
    n = F if n_frames is None else n_frames
    d_in = ctx.alloc(max(cubes.nbytes, 16))
    d_out = ctx.alloc((F * C + GUARD) * 4)
    try:
        d_in.upload(cubes)
        d_out.upload(np.full(F * C + GUARD, POISON, dtype=np.float32))
        rc = ctx.lib.mmw_micro_doppler(ctx.handle, d_in.at(first * V * S * C * 8), d_out.ptr, n, V, S, C, rx, lo, hi)
        return rc, d_out.download((F * C + GUARD,), np.float32).copy()
    finally:
        d_in.free()
        d_out.free()


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(os.path.join(GOLDEN, "micro_doppler.npz"), allow_pickle=False)
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as fh:
        ent = json.load(fh)[str(g["cfg"])]
    cm = ConfigManager()
    cm.load_cfg_text("\n".join(ent["lines"]) + "\n")
    return g, cm, (ent["expect"]["num_rx"], ent["expect"]["num_tx"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_raw_abi_on_marker_tones(shape):
    ctx = _lib.default_context()
    V, S, C = shape
    worst, inside = 0.0, 0
    for lo, hi in windows(S):
        cubes = tone_cubes(shape, lo, hi)
        for rx in sorted({0, V - 1}):
            rc, buf = run_abi(ctx, cubes, rx, lo, hi)
            assert rc == _lib.MMW_OK, ctx.lib.mmw_last_error()
            got = buf[:len(cubes) * C].reshape(len(cubes), C)
            assert np.all(buf[len(cubes) * C:] == POISON)
            for f, cube in enumerate(cubes):
                want, peak = expected(cube, rx, lo, hi)
                inside += want.max() == peak                    # the strongest target lies inside the window
                ratio = float(np.max(np.abs(got[f] - want))) / peak
                worst = max(worst, ratio)
                assert ratio <= SPEC_TOL, (shape, lo, hi, rx, f, ratio)
    print(f"micro_doppler {V}x{S}x{C}: worst |err| / peak {worst:.3e} (bar {SPEC_TOL:.0e}), {inside} frames with the peak inside")
    assert inside > 0


def test_rows_in_flight_do_not_change_a_bit():
    """4, 8 or 16 window rows per pass (the MMW_MD_KT switch) add the same terms in the same order."""
    ctx = _lib.default_context()
    shape, (lo, hi) = (3, 64, 32), (2, 40)
    cubes = tone_cubes(shape, lo, hi, F=3, seed=5)
    rc, base = run_abi(ctx, cubes, 1, lo, hi)
    assert rc == _lib.MMW_OK
    try:
        for kt in (4, 8, 16):
            ctx.set_option("MMW_MD_KT", kt)
            rc, buf = run_abi(ctx, cubes, 1, lo, hi)
            assert rc == _lib.MMW_OK and np.array_equal(buf, base), kt
    finally:
        ctx.set_option("MMW_MD_KT", None)


@pytest.mark.parametrize("shape,window", [((2, 40, 23), (3, 25)), ((2, 8, 130), (1, 6))], ids=["40x23", "8x130"])
def test_batch_rows_equal_single_frame_calls_bit_for_bit(shape, window):
    ctx = _lib.default_context()
    F, (V, S, C), (lo, hi) = 37, shape, window      # one workgroup per frame: 37 is no multiple of anything in the launch
    rng = np.random.default_rng(11)
    cubes = (np.round(40 * rng.standard_normal((F, V, S, C))) + 1j * np.round(40 * rng.standard_normal((F, V, S, C)))).astype(np.complex64)
    rc, buf = run_abi(ctx, cubes, V - 1, lo, hi)
    assert rc == _lib.MMW_OK, ctx.lib.mmw_last_error()
    got = buf[:F * C].reshape(F, C)
    assert np.all(got >= 0) and np.all(buf[F * C:] == POISON)           # every row written, nothing behind them
    for f in range(F):
        rc, one = run_abi(ctx, cubes, V - 1, lo, hi, n_frames=1, first=f)
        assert rc == _lib.MMW_OK
        assert np.array_equal(one[:C], got[f]) and np.all(one[C:] == POISON), f
    want, peak = expected(cubes[F - 1], V - 1, lo, hi)
    assert float(np.max(np.abs(got[F - 1] - want))) / peak <= SPEC_TOL


def test_fixture_processor_pipeline_history_and_raw_load():
    g, cm, (num_rx, num_tx) = fixture()
    cubes, H = g["cubes"], int(g["num_frames_history"])
    F, V, S, C = cubes.shape
    tr = g["target_ranges"].tolist()
    pipe = FramePipeline(cm, max_frames=F, shape=(V, S, C))
    worst = 0.0
    for i, rx in enumerate(int(r) for r in g["rx"]):
        proc = MicroDopplerProcessor(cm, target_ranges=tr, num_frames_history=H)
        col0 = []
        for f in range(F):
            buf = proc.process(cubes[f], rx_idx=rx)
            assert buf is proc.micro_doppler_resp and buf.shape == (C, H) and buf.dtype == np.float64
            for age in range(H):                                # column `age` holds frame f - age: that frame's peak scales its bar
                peak = g["peaks"][i, f - age] if f - age >= 0 else 1.0
                ratio = float(np.max(np.abs(buf[:, age] - g["buffers"][i, f][:, age]))) / peak
                worst = max(worst, ratio)
                assert ratio <= SPEC_TOL, (rx, f, age, ratio)
            col0.append(buf[:, 0].copy())
        pipe.load(cubes)
        rows = pipe.micro_doppler(target_ranges=tr, rx_idx=rx)
        assert rows.shape == (F, C) and rows.dtype == np.float64
        assert np.array_equal(rows, np.stack(col0))             # the same kernel: bit-identical to the processor's column 0
        assert np.array_equal(micro_doppler_history(rows, H), proc.micro_doppler_resp)
        assert float(np.max(np.abs(micro_doppler_history(rows, H) - g["buffers"][i, F - 1]))) <= SPEC_TOL * g["peaks"][i].max()
        # the rows left on the device are the rows downloaded
        d = pipe.micro_doppler_device(target_ranges=tr, rx_idx=rx)
        assert np.array_equal(d.download((F, C), np.float32).astype(np.float64), rows)
        # negative antenna indices count from the end, as they do in adc_cube[rx_idx]
        assert np.array_equal(pipe.micro_doppler(target_ranges=tr, rx_idx=rx - V), rows)
        # raw cubes [F, num_rx, S, num_tx * loops]: virtual antenna tx * num_rx + r is every num_tx-th chirp, from tx
        raw = np.zeros((F, num_rx, S, num_tx * C), dtype=np.complex64)
        for tx in range(num_tx):
            raw[:, :, :, tx::num_tx] = cubes[:, tx * num_rx:(tx + 1) * num_rx]
        pipe.load_raw(raw, num_tx)
        assert np.array_equal(pipe.cubes(), cubes)
        assert np.array_equal(pipe.micro_doppler(target_ranges=tr, rx_idx=rx), rows)
        # stream() chunks of 2 + 1 frames, concatenated
        small = FramePipeline(cm, max_frames=2, shape=(V, S, C))
        chunks = list(small.stream([cubes[:2], cubes[2:]], work=lambda p: p.micro_doppler(target_ranges=tr, rx_idx=rx)))
        assert np.array_equal(np.concatenate(chunks), rows)
        small.bufs.free()
    print(f"micro_doppler fixture 12x63x100: worst |err| / peak {worst:.3e} (bar {SPEC_TOL:.0e})")
    with pytest.raises(ValueError, match="no range bin"):
        pipe.micro_doppler(target_ranges=(2.3 * cm.range_res_m, 2.7 * cm.range_res_m))
    with pytest.raises(IndexError):
        pipe.micro_doppler(rx_idx=V)
    pipe.bufs.free()


def test_processor_on_degenerate_axes():
    """One chirp and one sample through the class, against the inline definition."""
    rng = np.random.default_rng(3)
    for (V, S, C), tr in (((2, 16, 1), [2, 9]), ((2, 1, 8), [0, 1.0])):
        cube = (rng.standard_normal((V, S, C)) + 1j * rng.standard_normal((V, S, C))).astype(np.complex64)
        proc = MicroDopplerProcessor(GridConfig(S, C), target_ranges=tr, num_frames_history=3)
        lo, hi = proc.rows
        assert (lo, hi) == ((2, 9) if S == 16 else (0, 0))
        out = proc.process(cube, rx_idx=1)
        want, peak = expected(cube, 1, lo, hi)
        assert out.shape == (C, 3) and float(np.max(np.abs(out[:, 0] - want))) / peak <= SPEC_TOL and not out[:, 1:].any()


def test_bad_arguments_launch_nothing():
    ctx = _lib.default_context()
    cubes = tone_cubes((2, 16, 8), 3, 5, F=2)
    F, V, S, C = cubes.shape
    bad = [dict(rx=-1), dict(rx=V), dict(lo=6, hi=5), dict(lo=-1, hi=3), dict(lo=3, hi=S), dict(lo=S, hi=S + 2), dict(n=-1),
           dict(V=0), dict(S=0), dict(C=0)]
    d_in = ctx.alloc(cubes.nbytes)
    d_out = ctx.alloc((F * C + GUARD) * 4)
    try:
        d_in.upload(cubes)
        d_out.upload(np.full(F * C + GUARD, POISON, dtype=np.float32))

        def call(n=F, V=V, S=S, C=C, rx=0, lo=3, hi=5, cubes_ptr=d_in.ptr, out_ptr=d_out.ptr, handle=ctx.handle):
            return ctx.lib.mmw_micro_doppler(handle, cubes_ptr, out_ptr, n, V, S, C, rx, lo, hi)
        for kw in bad + [dict(cubes_ptr=None), dict(out_ptr=None), dict(handle=None)]:
            assert call(**kw) == _lib.MMW_ERR_INVALID, kw
            assert len(ctx.lib.mmw_last_error()) > 0
        assert call(n=0) == _lib.MMW_OK                         # no frames: a successful no-op
        assert np.all(d_out.download((F * C + GUARD,), np.float32) == POISON)
        assert call() == _lib.MMW_OK                            # ... and the same buffers serve a good call
        got = d_out.download((F * C + GUARD,), np.float32)
        assert np.all(got[:F * C] >= 0) and np.all(got[F * C:] == POISON)
    finally:
        d_in.free()
        d_out.free()


def test_multi_device_form_on_one_device_equals_the_pipeline():
    g, cm, _ = fixture()
    cubes = g["cubes"]
    F, V, S, C = cubes.shape
    tr = g["target_ranges"].tolist()
    pipe = FramePipeline(cm, max_frames=F, shape=(V, S, C))
    pipe.load(cubes)
    want = pipe.micro_doppler(target_ranges=tr, rx_idx=11)
    mp = MultiDeviceFramePipeline(cm, max_frames=F, shape=(V, S, C), devices=[0])
    try:
        mp.load(cubes)
        got = mp.micro_doppler(target_ranges=tr, rx_idx=11)
    finally:
        mp.close()
    assert got.shape == (F, C) and got.dtype == np.float64 and np.array_equal(got, want)
    pipe.bufs.free()


def test_profile_family_is_registered():
    ctx = _lib.default_context()
    cubes = tone_cubes((2, 16, 8), 3, 5, F=2)
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        rc, _ = run_abi(ctx, cubes, 0, 3, 5)
        assert rc == _lib.MMW_OK
        ctx.sync()
        ms, n = ctx.profile_get("micro_doppler")
        assert n == 1 and ms > 0
    finally:
        ctx.profile_enable(False)
