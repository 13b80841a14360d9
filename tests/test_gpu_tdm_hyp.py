"""TDM-MIMO velocity unwrapping on the device: mmw_angle_argmax_tdm_hyp against the host twin of its float64 stage
(bit for bit) and the NumPy oracle of tests/tdm_hyp_cases.py (where decided) on the complex128 cells mmw_rd_cells64_at returns,
the float64 route on an all-tie batch, the given-hypothesis mode, the single-hypothesis hand-overs, mmw_tdm_unwrap_velocity
against NumPy, and FramePipeline / PointCloudGenerator / MultiDeviceFramePipeline with tdm_velocity_unwrap=True on folded targets.

Small shapes: 12 x 16 x 16, 12 x 16 x 7 and 12 x 32 x 128 (the largest phasor image: 9 rows of 128), four frames, cap 7 (one
partial workgroup) and 300 (two workgroups per frame, the second partial).  No kernel here caps its grid.
"""
import numpy as np
import pytest

import tdm_cases as tc
import tdm_hyp_cases as hc
from mmwave_radar_processing_amd import _lib, synth
from mmwave_radar_processing_amd.batch import (FramePipeline, MultiDeviceFramePipeline, tdm_hypothesis_table, tdm_phase_table,
                                               tdm_unwrapped_bin)
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.detectors import CaCFAR2D
from mmwave_radar_processing_amd.processors import PointCloudGenerator

from test_gpu_tdm_argmax import Resident, impulse_cubes
from test_tdm_hyp_cases_host import host_twin

pytestmark = pytest.mark.gpu
SENTINEL = -7
SHAPES = ((12, 16, 16), (12, 16, 7), (12, 32, 128))
CAPS = (7, 300)
LISTS = ([2, 3, 4, 5], list(range(8)), list(range(12)))      # NA = 4, 8, 16; two, two and three transmit slots
SLOTS, N_SLOTS = tc.default_slots(12, 4)


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


class ResidentHyp(Resident):
    """Resident of test_gpu_tdm_argmax with the hypothesis buffer [F][cap] int32."""

    def __init__(self, ctx, cubes, dets, counts):
        super().__init__(ctx, cubes, dets, counts)
        self.b["hyp"] = ctx.alloc(self.F * self.cap * 4)

    def hyp(self, ants, A, shift, table, given=None):
        """(d_idx, d_hyp, n_refined) of mmw_angle_argmax_tdm_hyp; given: the [F][cap] hypotheses handed in."""
        b, h = self.b, self.ctx.handle
        table = np.ascontiguousarray(table, dtype=np.complex128)
        b["idx"].upload(np.full((self.F, self.cap), SENTINEL, dtype=np.int32))
        b["hyp"].upload(np.full((self.F, self.cap), SENTINEL, dtype=np.int32) if given is None
                        else np.ascontiguousarray(given, dtype=np.int32))
        arr, n_ant = _lib.int_array(ants)
        n_ref = _lib.C.c_int(-1)
        _lib.check(self.ctx.lib.mmw_angle_argmax_tdm_hyp(h, b["cube"].ptr, b["l1"].ptr, b["rd"].ptr, b["dets"].ptr, b["counts"].ptr,
                                                         b["idx"].ptr, b["hyp"].ptr, int(given is not None), self.F, self.V, self.S,
                                                         self.C, self.cap, arr, n_ant, A, int(shift), table.ctypes.data, table.shape[0],
                                                         _lib.C.byref(n_ref)))
        return (b["idx"].download((self.F, self.cap), np.int32).copy(), b["hyp"].download((self.F, self.cap), np.int32).copy(),
                n_ref.value)


@pytest.fixture(scope="module", params=[(s, c) for s in SHAPES for c in CAPS], ids=lambda p: "x".join(map(str, p[0])) + f"-cap{p[1]}")
def noisy(request, ctx):
    shape, cap = request.param
    counts = [cap, 0, 5, cap + 9]
    cubes = hc.noisy_scene(7, shape, len(counts))
    dets, counts = tc.detection_lists(8, shape, counts, cap)
    with ResidentHyp(ctx, cubes, dets, counts) as r:
        yield r


@pytest.mark.parametrize("A,shift", [(64, 1), (16, 0)])
@pytest.mark.parametrize("ants", LISTS, ids=lambda a: f"n{len(a)}")
def test_twin_and_oracle_parity(noisy, ants, A, shift):
    table = tdm_hypothesis_table(ants, SLOTS, N_SLOTS, noisy.C)
    cells = noisy.cells64(ants)[noisy.live]
    cols = noisy.dets[..., 1][noisy.live]
    t_idx, t_hyp = host_twin(cells, cols, table, A, shift)
    o_idx, o_hyp, decided = hc.oracle(cells, cols, table, A, shift)
    got, hyp, n_ref = noisy.hyp(ants, A, shift, table)
    print(f"{noisy.live.sum()} live detections, {n_ref} re-evaluated in float64, {(~decided).sum()} excluded by the oracle")
    assert 0 <= n_ref <= noisy.live.sum()
    assert np.array_equal(got[noisy.live], t_idx) and np.array_equal(hyp[noisy.live], t_hyp)
    assert decided.mean() >= 0.99
    assert np.array_equal(got[noisy.live][decided], o_idx[decided]) and np.array_equal(hyp[noisy.live][decided], o_hyp[decided])
    assert np.all(got[~noisy.live] == SENTINEL) and np.all(hyp[~noisy.live] == SENTINEL)
    assert len(np.unique(hyp[noisy.live])) == N_SLOTS        # every hypothesis wins somewhere on these scenes
    # the hypothesis given: the deciding call's own indices, d_hyp left alone (dead slots and values out of range included)
    given = hyp.copy()
    g_idx, g_hyp, g_ref = noisy.hyp(ants, A, shift, table, given=given)
    assert np.array_equal(g_idx, got) and np.array_equal(g_hyp, given) and 0 <= g_ref <= noisy.live.sum()
    other = np.where(noisy.live, (hyp + 1) % N_SLOTS + N_SLOTS * (np.arange(noisy.cap)[None, :] % 2), 99).astype(np.int32)
    g_idx, g_hyp, _ = noisy.hyp(ants, A, shift, table, given=other)      # (odd slots: out of range, clamped to the last)
    w_idx, _ = host_twin(cells, cols, table, A, shift, given=np.clip(other[noisy.live], 0, N_SLOTS - 1))
    assert np.array_equal(g_idx[noisy.live], w_idx) and np.array_equal(g_hyp, other)
    assert np.all(g_idx[~noisy.live] == SENTINEL)


@pytest.mark.parametrize("shift", [0, 1])
def test_single_hypothesis_calls_hand_over(noisy, shift):
    A = 64
    # a list inside one slot: mmw_angle_argmax_exact, hypothesis 0
    for ants in ([8, 9, 10, 11], [5]):
        table = tdm_hypothesis_table(ants, SLOTS, N_SLOTS, noisy.C)
        got, hyp, n_got = noisy.hyp(ants, A, shift, table)
        want, n_want = noisy.exact(ants, A, shift)
        assert np.array_equal(got, want) and n_got == n_want
        assert np.all(hyp[noisy.live] == 0) and np.all(hyp[~noisy.live] == SENTINEL)
        given = np.full((noisy.F, noisy.cap), 2, dtype=np.int32)
        got, hyp, n_got = noisy.hyp(ants, A, shift, table, given=given)
        assert np.array_equal(got, want) and n_got == n_want and np.array_equal(hyp, given)
    # H == 1: mmw_angle_argmax_tdm on that table
    ants = LISTS[1]
    table = tdm_hypothesis_table(ants, SLOTS, N_SLOTS, noisy.C)
    got, hyp, n_got = noisy.hyp(ants, A, shift, table[:1])
    want, n_want = noisy.tdm(ants, A, shift, tdm_phase_table(ants, SLOTS, N_SLOTS, noisy.C))
    assert np.array_equal(got, want) and n_got == n_want
    assert np.all(hyp[noisy.live] == 0) and np.all(hyp[~noisy.live] == SENTINEL)
    for bad in (table[:0], np.ones((9,) + table.shape[1:], dtype=np.complex128)):       # H < 1, H > 8
        with pytest.raises(ValueError):
            noisy.hyp(ants, A, shift, bad)


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_all_tie_batch_goes_through_float64(ctx, shape):
    """Cells non-zero on slot-0 antennas only: every hypothesis multiplies them by one, the spectra tie bit for bit, the float32
    pass can decide none of them, and the float64 stage keeps hypothesis 0."""
    V, S, C = shape
    A, cap = 64, 300
    dets, counts = tc.detection_lists(3, shape, [cap, 0, 5, cap + 9], cap)
    amps = np.zeros(V, dtype=np.complex64)
    amps[:4] = [500.0 - 125.0j, 300.0 + 40.0j, -250.0 + 10.0j, 90.0 + 410.0j]
    ants = list(range(8))
    table = tdm_hypothesis_table(ants, SLOTS, N_SLOTS, C)
    with ResidentHyp(ctx, impulse_cubes(shape, amps, len(counts)), dets, counts) as r:
        for shift in (0, 1):
            got, hyp, n_ref = r.hyp(ants, A, shift, table)
            assert n_ref == r.live.sum()
            assert np.all(hyp[r.live] == 0) and np.all(hyp[~r.live] == SENTINEL) and np.all(got[~r.live] == SENTINEL)
            t_idx, t_hyp = host_twin(r.cells64(ants)[r.live], r.dets[..., 1][r.live], table, A, shift)
            assert np.array_equal(got[r.live], t_idx) and np.all(t_hyp == 0)


def test_noiseless_physics_batch(ctx):
    """One noiseless target per frame on every true Doppler bin of the extended range: k' is the true bin, the angle bin within 1."""
    num_rx, num_tx, S, loops, A = 4, 3, 16, 16, 64
    M = num_tx * loops
    truth = list(range(-(M // 2), M - M // 2))
    scenes = [hc.physics_scene(40 + kd % 3, kd, num_rx, num_tx, S, loops, A=A, shift=True) for kd in truth]
    cubes = np.stack([s[0] for s in scenes])
    dets = np.zeros((len(truth), 2, 2), dtype=np.int32)
    dets[:, 0] = [s[1] for s in scenes]
    counts = np.ones(len(truth), dtype=np.int32)
    ants = list(range(8))
    table = tdm_hypothesis_table(ants, SLOTS, N_SLOTS, loops)
    with ResidentHyp(ctx, cubes, dets, counts) as r:
        got, hyp, n_ref = r.hyp(ants, A, True, table)
    print(f"noiseless physics batch: {n_ref} of {len(truth)} detections re-evaluated in float64")
    assert np.array_equal(tdm_unwrapped_bin(dets[:, 0, 1], hyp[:, 0], N_SLOTS, loops), truth)
    d = np.abs(got[:, 0] - np.array([s[2] for s in scenes]))
    assert np.all(np.minimum(d, A - d) <= 1)
    assert np.all(got[:, 1] == SENTINEL) and np.all(hyp[:, 1] == SENTINEL)


@pytest.mark.parametrize("A,shift", [(64, 1), (16, 0)])
def test_float64_stage_equals_host_twin(ctx, A, shift):
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(21)
    for n_ant, C in ((1, 9), (3, 8), (8, 10), (12, 9), (16, 16)):
        ants = [v % 12 for v in range(n_ant)]
        table = tdm_hypothesis_table(ants, SLOTS, N_SLOTS, C)
        n = 203
        cells = rng.standard_normal((n, n_ant)) + 1j * rng.standard_normal((n, n_ant))
        cells[:8] = 0.0
        cells[:8, 0] = 2.0 + 1.0j                         # slot 0 only: exact ties between the hypotheses
        cells[8:12] = 1.0                                 # equal antennas
        cells[12, n_ant - 1] = np.nan
        cols = rng.integers(0, C, n).astype(np.int32)
        given = rng.integers(-2, N_SLOTS + 2, n).astype(np.int32)
        d_cells, d_cols, d_idx, d_hyp = ctx.alloc(cells.nbytes), ctx.alloc(cols.nbytes), ctx.alloc(n * 4), ctx.alloc(n * 4)
        try:
            d_cells.upload(cells)
            d_cols.upload(cols)
            for g in (None, given):
                t_idx, t_hyp = host_twin(cells, cols, table, A, shift, given=g)
                d_idx.upload(np.full(n, SENTINEL, dtype=np.int32))
                d_hyp.upload(np.full(n, SENTINEL, dtype=np.int32) if g is None else g)
                _lib.check(lib.mmw_angle_argmax_cells64_tdm_hyp(h, d_cells.ptr, d_cols.ptr, table.ctypes.data, N_SLOTS, d_idx.ptr,
                                                                d_hyp.ptr, int(g is not None), n, n_ant, C, A, shift))
                assert np.array_equal(d_idx.download((n,), np.int32), t_idx)
                assert np.array_equal(d_hyp.download((n,), np.int32), t_hyp)
                o_idx, o_hyp, decided = hc.oracle(cells, cols, table, A, shift, given=g)
                assert np.array_equal(t_idx[decided], o_idx[decided]) and np.array_equal(t_hyp[decided], o_hyp[decided])
        finally:
            for buf in (d_cells, d_cols, d_idx, d_hyp):
                buf.free()


@pytest.mark.parametrize("n_slots,C", [(3, 16), (2, 7), (4, 8)])
def test_unwrap_velocity_against_numpy(ctx, n_slots, C):
    F, cap, span = 5, 300, 7.25
    rng = np.random.default_rng(n_slots * 100 + C)
    counts = np.array([cap, 0, 5, cap + 9, -3], dtype=np.int32)
    points = rng.standard_normal((F, cap, 4))
    points[0, :4, 3] = [-0.0, 0.0, np.inf, 2.0 ** -1074]
    dets = np.stack([rng.integers(0, 50, (F, cap)), rng.integers(0, C, (F, cap))], axis=-1).astype(np.int32)
    dets[0, 10, 1], dets[0, 11, 1] = -1, C                   # outside the plane: column 0, as mmw_point_cloud reads it
    hyp = rng.integers(0, n_slots, (F, cap)).astype(np.int32)
    hyp[0, :4] = 0
    hyp[0, 20], hyp[0, 21] = -4, n_slots + 3                 # clamped
    live = np.arange(cap)[None, :] < np.clip(counts, 0, cap)[:, None]
    want = points.copy()
    c = np.where((dets[..., 1] >= 0) & (dets[..., 1] < C), dets[..., 1], 0)
    new_v = hc.unwrapped_velocity(points[..., 3].ravel(), c.ravel(), np.clip(hyp, 0, n_slots - 1).ravel(), n_slots, C, span)
    want[..., 3] = np.where(live, new_v.reshape(F, cap), points[..., 3])
    bufs = [ctx.alloc(points.nbytes), ctx.alloc(dets.nbytes), ctx.alloc(counts.nbytes), ctx.alloc(hyp.nbytes)]
    try:
        for buf, arr in zip(bufs, (points, dets, counts, hyp)):
            buf.upload(arr)
        _lib.check(ctx.lib.mmw_tdm_unwrap_velocity(ctx.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, F, cap, C, n_slots,
                                                   span))
        ctx.sync()
        got = bufs[0].download((F, cap, 4), np.float64)
    finally:
        for buf in bufs:
            buf.free()
    assert got.tobytes() == want.tobytes()
    m = hc.fold_count(c, np.clip(hyp, 0, n_slots - 1), n_slots, C)
    assert np.any(m[live] == 0) and np.any(m[live] > 0) and np.any(m[live] < 0)


# ------------------------------------------------------------------ end to end
AZ, EL = list(range(8)), [8, 9, 10, 11]
E2E_SHAPE = (12, 32, 16)
E2E_BINS = (5, 21, -11, -19, 13, -3)                        # true Doppler bins: folds m = 0, +1, -1, -1, +1, 0
E2E_R0 = 9


def make_cm(shape):
    cm = ConfigManager()
    cm.load_cfg_text(synth.synth_cfg_text(shape[1], shape[2], 3))
    return cm


@pytest.fixture(scope="module")
def folded():
    """One strong target per frame in light noise, each on its own true Doppler bin: (cubes, columns, folds, true angle bins)."""
    V, S, C = E2E_SHAPE
    cubes, cols, folds, bins = [], [], [], []
    for f, kd in enumerate(E2E_BINS):
        f_a = (-0.3, 0.17, 0.38, -0.12, 0.05, 0.29)[f]
        raw, b = synth.synth_tdm_targets(70 + f, 4, 3, S, C, [(200.0, E2E_R0 / S, kd / (3 * C), f_a)], noise_sigma=1.0,
                                         num_angle_bins=64, shift=True)
        k = int(hc.sym(kd, C))
        cubes.append(tc.deinterleave(raw, 3))
        cols.append(k + C // 2)
        folds.append((kd - k) // C)
        bins.append(int(b[0]))
    return np.stack(cubes), np.array(cols), np.array(folds), np.array(bins)


def target_rows(dets, cols):
    rows = []
    for d, c in zip(dets, cols):
        hit = np.nonzero((d[:, 0] == E2E_R0) & (d[:, 1] == c))[0]
        assert hit.size == 1, "the target must be detected for the test to mean anything"
        rows.append(int(hit[0]))
    return rows


def test_frame_pipeline_unwraps_folded_targets(ctx, folded):
    cubes, cols, folds, bins = folded
    assert folds.tolist() == [0, 1, -1, -1, 1, 0]
    F = len(cubes)
    cm = make_cm(E2E_SHAPE)
    common = dict(az_antenna_idxs=AZ, el_antenna_idxs=EL, det_capacity=64)
    cfar = lambda: CaCFAR2D((2, 1), (1, 1), 5e-2)               # noqa: E731
    on = FramePipeline(cm, F, E2E_SHAPE, cfar=cfar(), tdm_compensation=True, tdm_velocity_unwrap=True, **common)
    off = FramePipeline(cm, F, E2E_SHAPE, cfar=cfar(), tdm_compensation=True, tdm_velocity_unwrap=False, **common)
    ref = FramePipeline(cm, F, E2E_SHAPE, cfar=cfar(), tdm_compensation=True, **common)
    multi = MultiDeviceFramePipeline(cm, F, E2E_SHAPE, devices=[0], cfar=cfar(), tdm_compensation=True, tdm_velocity_unwrap=True,
                                     **common)
    try:
        for p in (on, off, ref, multi):
            p.load(cubes)
        clouds = on.point_clouds()
        rows = target_rows(on.dets, cols)
        span = 2.0 * cm.vel_max_m_s
        hyp, bins_k = on.tdm_hypotheses(), on.tdm_unwrapped_bins()
        assert hyp.shape == (F, 64) and hyp.dtype == np.int32 and on.tdm_hypotheses(1, 3).shape == (2, 64)
        for f, j in enumerate(rows):
            want_v = on.vel_bins[cols[f]] + float(folds[f]) * span if folds[f] else on.vel_bins[cols[f]]
            assert clouds[f][j, 3] == want_v
            assert bins_k[f, j] == E2E_BINS[f] == tdm_unwrapped_bin(cols[f], hyp[f, j], 3, E2E_SHAPE[2])
            d = abs(int(on.az_idx[f][j]) - bins[f])
            assert min(d, 64 - d) <= 1
            assert np.all(hyp[f, len(on.dets[f]):] == 0) and np.all(bins_k[f, len(on.dets[f]):] == 0)
        # every point: the v column is the table's value moved by the fold of its own hypothesis, the other columns as computed
        for f, d in enumerate(on.dets):
            n = len(d)
            want = hc.unwrapped_velocity(on.vel_bins[d[:, 1]], d[:, 1], hyp[f, :n], 3, E2E_SHAPE[2], span)
            assert clouds[f][:, 3].tobytes() == want.tobytes()
        on.point_clouds_device()
        for got, w in zip(on.fetch_point_clouds(), clouds):
            assert got.tobytes() == w.tobytes()
        # unwrapping off: the folded targets keep the folded speed and get a wrong bearing; the unfolded ones agree
        plain = off.point_clouds()
        for f, j in enumerate(rows):
            assert np.array_equal(off.dets[f], on.dets[f])
            d = abs(int(off.az_idx[f][j]) - bins[f])
            if folds[f]:
                assert plain[f][j, 3] == off.vel_bins[cols[f]] != clouds[f][j, 3]
                assert min(d, 64 - d) > 1
            else:
                assert np.array_equal(plain[f][j], clouds[f][j])
        # the keyword left out: bit-identical to the keyword off
        base = ref.point_clouds()
        for a, b in zip(plain, base):
            assert a.tobytes() == b.tobytes()
        assert off.n_refined == ref.n_refined
        for got, w in zip(multi.point_clouds(), clouds):
            assert got.tobytes() == w.tobytes()
        assert multi.n_refined == on.n_refined
    finally:
        for p in (on, off, ref):
            p.bufs.free()
        for p in multi.parts:
            p.bufs.free()


def test_point_cloud_generator_unwraps_folded_targets(ctx, folded):
    cubes, cols, folds, bins = folded
    cm = make_cm(E2E_SHAPE)
    pipe = FramePipeline(cm, len(cubes), E2E_SHAPE, cfar=CaCFAR2D((2, 1), (1, 1), 5e-2), az_antenna_idxs=AZ, el_antenna_idxs=EL,
                         det_capacity=64, tdm_compensation=True, tdm_velocity_unwrap=True)
    pcg = PointCloudGenerator(cm, AZ, EL, detector_params={"cfar_type": "ca_cfar_2d", "cfar_params": {
        "num_train": (2, 1), "num_guard": (1, 1), "pfa": 5e-2}}, tdm_compensation=True, tdm_velocity_unwrap=True)
    try:
        pipe.load(cubes)
        clouds = pipe.point_clouds()
        hyp = pipe.tdm_hypotheses()
        for f, cube in enumerate(cubes):
            pc = pcg.process(cube)
            assert pc.tobytes() == clouds[f].tobytes()
            assert pcg.tdm_hypotheses.dtype == np.int32 and np.array_equal(pcg.tdm_hypotheses, hyp[f, :len(pc)])
    finally:
        pipe.bufs.free()
