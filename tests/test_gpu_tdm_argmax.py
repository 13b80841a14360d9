"""TDM-MIMO Doppler phase compensation on the device: mmw_angle_argmax_tdm against the NumPy oracle of
tests/tdm_cases.py on the complex128 cells mmw_rd_cells64_at returns, its single-slot contract against mmw_angle_argmax_exact,
the undecided route, the float64 stage against its host twin, and FramePipeline(tdm_compensation=True).

Tiny shapes only (12 x 16 x 8, 12 x 15 x 10, 12 x 16 x 9), at most 8 frames, cap <= 64.  Neither kernel caps its grid
(k_argmax_tdm: cap / 256 workgroups per frame, k_argmax64_cells_tdm: one wave per row), so there is no second trip to cover.
"""
import numpy as np
import pytest

import tdm_cases as tc
from mmwave_radar_processing_amd import _lib, synth
from mmwave_radar_processing_amd.batch import FramePipeline, tdm_phase_table
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.detectors import CaCFAR2D
from mmwave_radar_processing_amd.processors.range_doppler_detection import RangeDopplerDetectorSequential
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu
SENTINEL = -7
SHAPES = ((12, 16, 8), (12, 15, 10), (12, 16, 9))
CAP = 24
COUNTS = [0, 5, CAP, CAP + 9, 1, -3, 17, CAP]          # empty, partial, full, above cap, negative
# one list per NA instantiation (4 / 8 / 16 / 32), each spanning more than one transmit slot
LISTS = ([2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6, 7], list(range(12)), list(range(12)) + list(range(8)))
SLOTS, N_SLOTS = tc.default_slots(12, 4)


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


class Resident:
    """Cubes [F][V][S][C], a detection list, the float32 range-Doppler cube and the plane norms on the device."""

    def __init__(self, ctx, cubes, dets, counts):
        self.ctx, self.cubes, self.dets, self.counts = ctx, cubes, dets, counts
        self.F, self.V, self.S, self.C = cubes.shape
        self.cap = dets.shape[1]
        n, slots = cubes.nbytes, self.F * self.cap
        self.b = dict(cube=ctx.alloc(n), rd=ctx.alloc(n), l1=ctx.alloc(self.F * self.V * 4), dets=ctx.alloc(slots * 8),
                      counts=ctx.alloc(self.F * 4), idx=ctx.alloc(slots * 4), cells=ctx.alloc(slots * 32 * 16))
        b = self.b
        b["cube"].upload(cubes)
        b["dets"].upload(dets)
        b["counts"].upload(counts)
        _lib.check(ctx.lib.mmw_range_doppler(ctx.handle, b["cube"].ptr, b["rd"].ptr, None, self.F, self.V, self.S, self.C))
        _lib.check(ctx.lib.mmw_plane_l1(ctx.handle, b["cube"].ptr, b["l1"].ptr, self.F, self.V, self.S, self.C))
        self.live = np.arange(self.cap)[None, :] < np.clip(counts, 0, self.cap)[:, None]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for buf in self.b.values():
            buf.free()

    def _call(self, fn, ants, A, shift, *extra):
        b, h = self.b, self.ctx.handle
        b["idx"].upload(np.full((self.F, self.cap), SENTINEL, dtype=np.int32))
        arr, n_ant = _lib.int_array(ants)
        n_ref = _lib.C.c_int(-1)
        _lib.check(fn(h, b["cube"].ptr, b["l1"].ptr, b["rd"].ptr, b["dets"].ptr, b["counts"].ptr, b["idx"].ptr, self.F, self.V,
                      self.S, self.C, self.cap, arr, n_ant, A, int(shift), *extra, _lib.C.byref(n_ref)))
        return b["idx"].download((self.F, self.cap), np.int32), n_ref.value

    def tdm(self, ants, A, shift, table):
        table = np.ascontiguousarray(table, dtype=np.complex128)
        return self._call(self.ctx.lib.mmw_angle_argmax_tdm, ants, A, shift, table.ctypes.data)

    def exact(self, ants, A, shift):
        return self._call(self.ctx.lib.mmw_angle_argmax_exact, ants, A, shift)

    def cells64(self, ants):
        """complex128 cells [F][cap][n_ant] of the listed detections (direct route), zeros elsewhere."""
        b = self.b
        arr, n_ant = _lib.int_array(ants)
        b["cells"].zero()
        _lib.check(self.ctx.lib.mmw_rd_cells64_at(self.ctx.handle, b["cube"].ptr, b["dets"].ptr, b["counts"].ptr, b["cells"].ptr,
                                                  self.F, self.V, self.S, self.C, self.cap, arr, n_ant, _lib.CELLS64_DIRECT))
        return b["cells"].download((self.F, self.cap, n_ant), np.complex128)

    def oracle(self, ants, A, shift, table):
        cells = self.cells64(ants)[self.live]
        cols = self.dets[..., 1][self.live]
        return tc.oracle_argmax(cells, cols, table, A, shift)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def noisy(request, ctx):
    shape = request.param
    cubes = tc.noisy_scene(7, shape, len(COUNTS))
    dets, counts = tc.detection_lists(8, shape, COUNTS, CAP)
    with Resident(ctx, cubes, dets, counts) as r:
        yield r


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("A", [16, 64])
@pytest.mark.parametrize("ants", LISTS, ids=lambda a: f"n{len(a)}")
def test_oracle_parity(noisy, ants, A, shift):
    if len(ants) > A:
        with pytest.raises(ValueError):
            noisy.tdm(ants, A, shift, tdm_phase_table(ants, SLOTS, N_SLOTS, noisy.C))
        return
    table = tdm_phase_table(ants, SLOTS, N_SLOTS, noisy.C)
    assert not tc.common_phase(table)
    want, decided = noisy.oracle(ants, A, shift, table)
    got, n_ref = noisy.tdm(ants, A, shift, table)
    assert decided.mean() >= 0.99
    assert 0 <= n_ref <= noisy.live.sum()
    assert np.array_equal(got[noisy.live][decided], want[decided])
    assert np.all(got[~noisy.live] == SENTINEL)
    plain, _ = noisy.oracle(ants, A, shift, None)
    assert np.any(plain != want)            # the compensation is not a no-op on these scenes


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("A", [16, 64])
def test_single_slot_lists_are_bit_identical_to_the_exact_entry(noisy, A, shift):
    for ants in ([8, 9, 10, 11], [0, 1, 2, 3], [5]):
        table = tdm_phase_table(ants, SLOTS, N_SLOTS, noisy.C)
        got, n_got = noisy.tdm(ants, A, shift, table)
        want, n_want = noisy.exact(ants, A, shift)
        assert np.array_equal(got, want) and n_got == n_want
    # a slot list of zeros: the table is all ones for any antenna list
    ants = LISTS[1]
    got, n_got = noisy.tdm(ants, A, shift, tdm_phase_table(ants, [0] * 12, 1, noisy.C))
    want, n_want = noisy.exact(ants, A, shift)
    assert np.array_equal(got, want) and n_got == n_want


def impulse_cubes(shape, amps, frames):
    """A single sample (s0, c0) per antenna plane: every range-Doppler cell of antenna v is amps[v] times one common factor."""
    V, S, C = shape
    cubes = np.zeros((frames, V, S, C), dtype=np.complex64)
    cubes[:, :, S // 2 - 1, C // 2 - 1] = np.asarray(amps, dtype=np.complex64)[None, :]
    return cubes


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_undecided_route(ctx, shape):
    """Cubes whose bins tie after compensation: one non-zero antenna (every bin the same value bit for bit), and a mirrored pair
    -- two antennas of different slots whose compensated cells sit 4e-6 rad off the midpoint between two bins: far inside the
    float32 bound, decided by 1e-7 of the magnitude in float64."""
    V, S, C = shape
    A, frames, cap = 64, 3, 16
    dets, counts = tc.detection_lists(3, shape, [cap, 7, cap + 1], cap)
    # ---- one non-zero antenna, first of the list
    amps = np.zeros(V, dtype=np.complex64)
    amps[3] = 500.0 - 125.0j
    ants = [3, 4, 5, 6]
    table = tdm_phase_table(ants, SLOTS, N_SLOTS, C)
    with Resident(ctx, impulse_cubes(shape, amps, frames), dets, counts) as r:
        for shift in (0, 1):
            got, n_ref = r.tdm(ants, A, shift, table)
            want, decided = r.oracle(ants, A, shift, table)
            assert n_ref == r.live.sum() and decided.all()
            assert np.all(want == 0) and np.array_equal(got[r.live], want)
            assert np.all(got[~r.live] == SENTINEL)
    # ---- mirrored pair: every detection of the list shares the Doppler column c, so one pair of amplitudes serves them all
    c = C // 2 + 2
    dets[..., 1] = c
    dets[..., 0] = np.arange(cap)[None, :] % S
    ants = [3, 4]
    table = tdm_phase_table(ants, SLOTS, N_SLOTS, C)
    amps = np.zeros(V, dtype=np.complex64)
    amps[3] = 1000.0
    amps[4] = np.complex64(1000.0 * np.conj(table[1, c]) * np.exp(1j * (np.pi * (2 * 9 + 1) / A + 4e-6)))
    with Resident(ctx, impulse_cubes(shape, amps, frames), dets, counts) as r:
        for shift in (0, 1):
            got, n_ref = r.tdm(ants, A, shift, table)
            want, decided = r.oracle(ants, A, shift, table)
            assert n_ref > 0 and decided.all()
            assert np.array_equal(got[r.live], want)
            assert set(np.unique(want)) <= {(9 + 32 * shift) % A, (10 + 32 * shift) % A}


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("A", [16, 64])
def test_float64_stage_equals_host_twin(ctx, A, shift):
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(21)
    for n_ant, C in ((1, 9), (3, 8), (8, 10), (12, 9), (16, 16)):
        ants = [v % 12 for v in range(n_ant)]
        table = tdm_phase_table(ants, SLOTS, N_SLOTS, C)
        n = 203
        cells = rng.standard_normal((n, n_ant)) + 1j * rng.standard_normal((n, n_ant))
        cells[:8] = 0.0
        cells[:8, 0] = 2.0 + 1.0j                         # exact ties
        cells[8:12] = 1.0                                 # equal antennas
        cells[12, n_ant - 1] = np.nan
        cols = rng.integers(0, C, n).astype(np.int32)
        twin = np.full(n, SENTINEL, dtype=np.int32)
        _lib.check(lib.mmw_diag_angle_argmax_tdm_host(cells.ctypes.data, cols.ctypes.data, table.ctypes.data, twin.ctypes.data, n,
                                                      n_ant, C, A, shift))
        d_cells, d_cols, d_idx = ctx.alloc(cells.nbytes), ctx.alloc(cols.nbytes), ctx.alloc(n * 4)
        try:
            d_cells.upload(cells)
            d_cols.upload(cols)
            d_idx.upload(np.full(n, SENTINEL, dtype=np.int32))
            _lib.check(lib.mmw_angle_argmax_cells64_tdm(h, d_cells.ptr, d_cols.ptr, table.ctypes.data, d_idx.ptr, n, n_ant, C, A, shift))
            got = d_idx.download((n,), np.int32)
        finally:
            for buf in (d_cells, d_cols, d_idx):
                buf.free()
        assert np.array_equal(got, twin)
        want, decided = tc.oracle_argmax(cells, cols, table, A, shift)
        assert np.array_equal(got[decided], want[decided])


# ------------------------------------------------------------------ FramePipeline
AZ, EL = [0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11]
SEQ = ("os_cfar_1d", {"num_train": 3, "num_guard": 1, "rho": 0.6, "alpha": 2},
       "os_cfar_1d", {"num_train": 2, "num_guard": 1, "rho": 0.7, "alpha": 2})


def make_cm(shape):
    cm = ConfigManager()
    cm.load_cfg_text(synth.synth_cfg_text(shape[1], shape[2], 3))
    return cm


def mode_kwargs(cm, mode):
    if mode == "cfar":
        return dict(cfar=CaCFAR2D((2, 1), (1, 1), 5e-2))
    rk, rp, vk, vp = SEQ
    return dict(sequential=RangeDopplerDetectorSequential(cm, rng_cfar_type=rk, rng_cfar_params=rp, vel_cfar_type=vk,
                                                          vel_cfar_params=vp))


def oracle_clouds(pipe, cubes, dets):
    out = []
    for f, d in enumerate(dets):
        if d.shape[0] == 0:
            out.append(np.empty((0, 4)))
            continue
        cells = tc.cells_of(cubes[f], d)
        ang = []
        for ants, shift in ((AZ, pipe.shift_az), (EL, pipe.shift_el)):
            table = tdm_phase_table(ants, SLOTS, N_SLOTS, pipe.C)
            idx, decided = tc.oracle_argmax(cells[:, ants], d[:, 1], table, pipe.A, shift)
            assert decided.all()
            ang.append(pipe.angle_bins[idx])
        az, el = ang
        rng, vel = pipe.range_bins[d[:, 0]], pipe.vel_bins[d[:, 1]]
        out.append(np.column_stack((rng * np.cos(el) * np.cos(az), rng * np.cos(el) * np.sin(az), rng * np.sin(el), vel)))
    return out


@pytest.mark.parametrize("mode", ["cfar", "sequential"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frame_pipeline(ctx, shape, mode):
    cm = make_cm(shape)
    cubes = tc.noisy_scene(31, shape, 6, noise_sigma=1.0)
    common = dict(az_antenna_idxs=AZ, el_antenna_idxs=EL, det_capacity=64)
    on = FramePipeline(cm, 6, shape, tdm_compensation=True, **common, **mode_kwargs(cm, mode))
    off = FramePipeline(cm, 6, shape, tdm_compensation=False, **common, **mode_kwargs(cm, mode))
    ref = FramePipeline(cm, 6, shape, **common, **mode_kwargs(cm, mode))
    try:
        for p in (on, off, ref):
            p.load(cubes)
        clouds = on.point_clouds()
        dets = on.dets
        assert sum(d.shape[0] for d in dets) >= 6, "the scene must produce detections for the test to mean anything"
        want = oracle_clouds(on, cubes, dets)
        for got, w in zip(clouds, want):
            assert got.shape == w.shape and np.array_equal(got, w)
        on.point_clouds_device()
        for got, w in zip(on.fetch_point_clouds(), clouds):
            assert np.array_equal(got, w)
        plain, base = off.point_clouds(), ref.point_clouds()
        for a, b in zip(plain, base):
            assert np.array_equal(a, b)
        assert off.n_refined == ref.n_refined
        for a, b in zip(off.dets, dets):
            assert np.array_equal(a, b)                     # the detections do not depend on the option
        assert any(not np.array_equal(a, b) for a, b in zip(plain, clouds))     # ... the bearings do
    finally:
        for p in (on, off, ref):
            p.bufs.free()
