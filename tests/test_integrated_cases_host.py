"""Antenna-integrated CFAR detection without a GPU: the conditions the GPU test (test_gpu_integrated_detect.py) rests on, asserted
on the NumPy restatement of tests/integrated_cases.py, and the argument errors of FramePipeline(integrate_rx=...).

| test                       | what it establishes                                                                                   |
|----------------------------|-------------------------------------------------------------------------------------------------------|
| margin                     | no valid cell of any case sits within 1e-9 (relative) of its threshold, so the device's detections can |
|                            | be demanded identical; the worst-case float64 error bound of P stays below every cell's distance too    |
| every case detects         | a case without detections would compare empty lists                                                    |
| weak target                | the 12-antenna power plane finds the cell the antenna-0 plane (|RD| and [0] power) misses              |
| order of the list          | another order of the same antennas changes P by rounding only                                          |
| argument errors            | every refused integrate_rx= raises ValueError before a device is touched                               |
| binding                    | the two entry points are bound, and route through the keyword only                                     |
"""
import numpy as np
import pytest

import integrated_cases as ic
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline
from oracle import oracle_np as O

IDS = [c.name for c in ic.CASES]


@pytest.mark.parametrize("name", IDS)
def test_margin_and_detections_of_every_case(name):
    c, ref = ic.BY_NAME[name], ic.reference(name)
    counts = [len(d) for d in ref.dets]
    print(f"{name}: margin {ref.margin:.3e}, detections per frame {counts}")
    assert ref.margin >= ic.MARGIN
    assert max(counts) > 0
    # even the worst-case error bound the GPU test allows P (L1-scaled: far above the real error) cannot move a cell of these seeds
    # across its threshold
    for f in range(len(c.seeds)):
        cube, rd, thr = ic.cubes(c.shape, c.seeds)[f], ic.rd_planes(c.shape, c.seeds)[f], ref.thr[f]
        ok = np.isfinite(thr) & (thr > 0)
        share = float(np.max(ic.power_bound(cube, rd, c.ants)[ok] / np.abs(ref.power[f][ok] - thr[ok])))
        assert share < 1.0, (f, share)


def test_case_list_reaches_every_route_and_list():
    routes = {c.route for c in ic.CASES}
    assert routes == {"persistent", "per_antenna_fused_shape", "per_antenna_lds", "per_antenna_two_pass"}
    by_shape = {}
    for c in ic.CASES:
        by_shape.setdefault(c.shape + (len(c.seeds),), set()).add(c.ants)
    for key, lists in by_shape.items():
        V = key[0]
        assert tuple(range(V)) in lists and (0,) in lists and any(list(a) != sorted(a) for a in lists), key
    assert {c.cfar[0] for c in ic.CASES} == {"ca", "os"}
    assert {(c.shape, len(c.seeds)) for c in ic.CASES} == {((12, 256, 128), 9), ((12, 256, 128), 3), ((12, 63, 70), 2),
                                                         ((12, 64, 64), 2), ((4, 512, 64), 2)}


def test_weak_target_is_found_by_integration_only():
    cube = ic.weak_cube()
    rd = O.range_doppler(cube)
    cell = np.array(ic.WEAK_CELL)
    _, dets_all = ic.cfar(ic.power(rd, list(range(12))), ic.CA)
    _, dets_one = ic.cfar(ic.power(rd, [0]), ic.CA)
    dets_mag = O.rd_detect_2d(cube)[2]
    has = lambda d: bool(len(d)) and bool(np.any(np.all(np.asarray(d) == cell, axis=1)))
    assert has(dets_all) and not has(dets_one) and not has(dets_mag)


def test_list_order_changes_rounding_only():
    c = ic.BY_NAME["256x128_f3-perm-ca"]
    rd = ic.rd_planes(c.shape, c.seeds)
    a, b = ic.power(rd, [7, 2, 9]), ic.power(rd, [2, 7, 9])
    assert np.max(np.abs(a - b) / a) <= 4 * 2.0 ** -53


class _NotADetector:
    pass


@pytest.mark.parametrize("bad", [[], [12], [-1], [0, 0], [3, 1, 3], [1.0], ["0"], [True], 5, list(range(40))],
                         ids=["empty", "too_large", "negative", "twice", "twice_apart", "float", "str", "bool", "scalar", "too_many"])
def test_refused_lists_raise_value_error(bad):
    with pytest.raises(ValueError, match="integrate_rx"):
        FramePipeline(None, 2, (12, 64, 64), integrate_rx=bad)


@pytest.mark.parametrize("other", ["ground", "sequential"])
def test_integrate_rx_with_another_detector_raises(other):
    with pytest.raises(ValueError, match="integrate_rx"):
        FramePipeline(None, 2, (12, 64, 64), integrate_rx=[0, 1], **{other: _NotADetector()})


def test_entry_points_are_bound_and_power_needs_the_keyword():
    for name, n_args in (("mmw_range_doppler_power64", 9), ("mmw_detect_batch_integrated", 22)):
        assert name in _lib.EXPORTED and len(_lib._SIGNATURES[name]) == n_args
    assert len(_lib._SIGNATURES["mmw_detect_batch_integrated"]) == len(_lib._SIGNATURES["mmw_detect_batch"]) + 2
    pipe = FramePipeline.__new__(FramePipeline)
    pipe.integrate_rx = None
    with pytest.raises(ValueError, match="integrate_rx"):
        pipe.integrated_power_device()
    assert callable(MultiDeviceFramePipeline.integrated_power)


def test_multi_device_joins_power_planes_in_frame_order():
    """The split / join logic on host-only fake parts (the pattern of test_sharding_cpu.py): every part returns planes tagged
    with its global frame numbers."""
    class Part:
        def __init__(self, device, n):
            self.lo = 0

        def load(self, cubes):
            self.tags = cubes[:, 0, 0, 0].real.astype(np.float64)

        def integrated_power(self):
            return self.tags[:, None, None] * np.ones((1, 4, 4))

    F = 7
    mp = MultiDeviceFramePipeline(None, F, (2, 4, 4), devices=[0, 1, 2], part_factory=Part, integrate_rx=[0, 1])
    cubes = np.zeros((F, 2, 4, 4), dtype=np.complex64)
    cubes[:, 0, 0, 0] = np.arange(F)
    mp.load(cubes)
    out = mp.integrated_power()
    assert out.shape == (F, 4, 4) and np.array_equal(out[:, 0, 0], np.arange(F))
