"""Host-side pieces of FramePipeline(ground=...): what it refuses (no device needed), the vectorised ground gate and the
Altimeter's sequence scan."""
import numpy as np
import pytest

from mmwave_radar_processing_amd import synth
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline, ground_gates
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.detectors import CaCFAR2D, OsCFAR1D
from mmwave_radar_processing_amd.processors.altimeter import GroundLock
from mmwave_radar_processing_amd.processors.range_doppler_detection import RangeDopplerGroundDetector
from mmwave_radar_processing_amd.processors.range_doppler_detection.range_doppler_ground_detector import slant_gate

ALT = {"min_altitude_m": 0.6, "zoom_search_region_m": 0.2, "altitude_search_limit_m": 0.6, "range_bias": 0.03,
       "precise_est_enabled": True}
VEL = {"num_train": 12, "num_guard": 4, "rho": 0.5, "alpha": 6}
SHAPE = (12, 256, 128)


def make_cm():
    cm = ConfigManager()
    cm.load_cfg_text(synth.SYNTH_CFG_256x128x12)
    return cm


def ground(cm, **kw):
    params = dict(vel_cfar_type="os_cfar_1d", vel_cfar_params=VEL, altimeter_params=ALT)
    params.update(kw)
    return RangeDopplerGroundDetector(cm, **params)


def test_refuses_a_velocity_detector_with_its_own_thresholds():
    class MyCFAR(OsCFAR1D):
        def _compute_thresholds(self, x):
            return np.full(len(x), 1.0), np.zeros(len(x))
    cm = make_cm()
    det = ground(cm)
    det.vel_detector = MyCFAR(**VEL)
    with pytest.raises(ValueError, match="own thresholds"):
        FramePipeline(cm, 4, SHAPE, ground=det)


def test_refuses_a_2d_velocity_key():
    cm = make_cm()
    det = ground(cm, vel_cfar_type="ca_cfar_2d", vel_cfar_params={"num_train": (4, 4), "num_guard": (2, 2), "pfa": 1e-5})
    with pytest.raises(ValueError, match="not a 1-D CFAR"):
        FramePipeline(cm, 4, SHAPE, ground=det)


def test_refuses_ground_with_cfar_and_on_several_devices():
    cm = make_cm()
    with pytest.raises(ValueError, match="not both"):
        FramePipeline(cm, 4, SHAPE, cfar=CaCFAR2D((4, 4), (2, 2), 1e-5), ground=ground(cm))
    with pytest.raises(ValueError, match="cannot take ground"):
        MultiDeviceFramePipeline(cm, 4, SHAPE, devices=[0, 1], part_factory=lambda d, n: object(), ground=ground(cm))
    with pytest.raises(ValueError, match="RangeDopplerGroundDetector"):
        FramePipeline(cm, 4, SHAPE, ground=object())


def test_ground_gates_equal_slant_gate():
    det = ground(make_cm())
    rb = det.range_bins
    alts = np.concatenate([np.random.default_rng(3).uniform(-1.0, rb[-1] + 2.0, 3000), rb, rb + rb[1] / 2, [0.0, 1e-6]])
    gates = ground_gates(rb, alts)
    assert gates.dtype == np.int32 and gates.shape == (alts.size, 2)
    for a, (near, far) in zip(alts, gates):
        np.testing.assert_array_equal(np.arange(near, far + 1), slant_gate(rb, a))


def test_lock_advance_is_the_frame_by_frame_step():
    """advance() over precomputed candidate lists == admit() frame by frame as Altimeter.process applies it, through
    locking, losing and regaining the gate (random candidate lists, several zoom lists per frame)."""
    rng = np.random.default_rng(5)
    F = 400
    truth = np.concatenate([np.linspace(0.7, 4.0, 150), np.linspace(8.0, 3.5, 150), np.linspace(3.5, 6.0, 100)])
    coarse, fine = [], []
    for f in range(F):
        n = int(rng.integers(0, 4))
        c = list(truth[f] + rng.normal(0, 0.3, n)) if n else []
        coarse.append(c)
        fine.append([list(x + rng.normal(0, 0.1, int(rng.integers(0, 3)))) for x in c] + [[]] * (3 - n))
    for precise in (False, True):
        lock = GroundLock(0.6, 0.6, 0.03)
        got = lock.advance(coarse, fine if precise else None)
        ref = GroundLock(0.6, 0.6, 0.03)
        want = []
        for f in range(F):
            hit = ref.admit(np.array(coarse[f]))
            if hit is not None and precise:
                hit = ref.admit(np.array(fine[f][coarse[f].index(hit)]))
            if hit is not None:
                ref.accept(hit)
            want.append(ref.reported_m)
        assert got == want and lock.measured_m == ref.measured_m
        moves = np.abs(np.diff(got)) > 0
        assert moves.sum() > 20 and (~moves).sum() > 20
