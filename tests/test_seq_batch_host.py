"""Host-side pieces of FramePipeline(sequential=...): what it refuses (no device needed), the sharded plumbing with fake
parts, and the ABI revision 7 entries in the header and the ctypes table."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mmwave_radar_processing_amd import _lib, synth
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline, shard_bounds
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.detectors import CaCFAR2D, OsCFAR1D
from mmwave_radar_processing_amd.processors.range_doppler_detection import (RangeDopplerDetectorSequential,
                                                                           RangeDopplerGroundDetector)
from test_sharding_cpu import _FakePart

RNG = {"num_train": 5, "num_guard": 3, "rho": 0.6, "alpha": 2}
VEL = {"num_train": 5, "num_guard": 2, "rho": 0.7, "alpha": 3}
SHAPE = (12, 256, 128)
NEW_ENTRIES = ("mmw_seq_rows", "mmw_seq_detect", "mmw_seq_detect_plane", "mmw_seq_route")


def make_cm():
    cm = ConfigManager()
    cm.load_cfg_text(synth.SYNTH_CFG_256x128x12)
    return cm


def sequential(cm, **kw):
    params = dict(rng_cfar_type="os_cfar_1d", rng_cfar_params=RNG, vel_cfar_type="os_cfar_1d", vel_cfar_params=VEL)
    params.update(kw)
    return RangeDopplerDetectorSequential(cm, **params)


def ground(cm):
    return RangeDopplerGroundDetector(cm, vel_cfar_type="os_cfar_1d", vel_cfar_params={"num_train": 12, "num_guard": 4, "rho": 0.5,
                                                                                      "alpha": 6},
                                      altimeter_params={"min_altitude_m": 0.6, "zoom_search_region_m": 0.2,
                                                        "altitude_search_limit_m": 0.6, "range_bias": 0.0,
                                                        "precise_est_enabled": False})


class MyCFAR(OsCFAR1D):
    def _compute_thresholds(self, x):
        return np.full(len(x), 1.0), np.zeros(len(x))


@pytest.mark.parametrize("which", ["rng_detector", "vel_detector"])
def test_refuses_a_detector_with_its_own_thresholds(which):
    cm = make_cm()
    det = sequential(cm)
    setattr(det, which, MyCFAR(**VEL))
    role = "range" if which == "rng_detector" else "velocity"
    with pytest.raises(ValueError, match=rf"sequential=: the {role} detector MyCFAR computes its own thresholds.*per-frame API"):
        FramePipeline(cm, 4, SHAPE, sequential=det)


@pytest.mark.parametrize("which", ["rng", "vel"])
def test_refuses_a_2d_key(which):
    cm = make_cm()
    kw = {f"{which}_cfar_type": "ca_cfar_2d", f"{which}_cfar_params": {"num_train": (4, 4), "num_guard": (2, 2), "pfa": 1e-5}}
    with pytest.raises(ValueError, match=r"sequential=: .*not a 1-D CFAR.*per-frame API"):
        FramePipeline(cm, 4, SHAPE, sequential=sequential(cm, **kw))


def test_refuses_sequential_with_cfar_or_ground_and_a_foreign_object():
    cm = make_cm()
    with pytest.raises(ValueError, match="not several"):
        FramePipeline(cm, 4, SHAPE, cfar=CaCFAR2D((4, 4), (2, 2), 1e-5), sequential=sequential(cm))
    with pytest.raises(ValueError, match="not several"):
        FramePipeline(cm, 4, SHAPE, ground=ground(cm), sequential=sequential(cm))
    with pytest.raises(ValueError, match="RangeDopplerDetectorSequential"):
        FramePipeline(cm, 4, SHAPE, sequential=object())
    with pytest.raises(ValueError, match="RangeDopplerDetectorSequential"):
        FramePipeline(cm, 4, SHAPE, sequential=ground(cm))


def test_several_devices_take_sequential_and_still_refuse_ground():
    cm = make_cm()
    with pytest.raises(ValueError, match="cannot take ground"):
        MultiDeviceFramePipeline(cm, 4, SHAPE, devices=[0, 1], part_factory=lambda d, n: object(), ground=ground(cm))
    shape, world, n_frames = (2, 2, 2), 3, 10
    mp = MultiDeviceFramePipeline(cm, max_frames=16, shape=shape, devices=list(range(world)),
                                  part_factory=lambda d, n: _FakePart(d, n, shape), sequential=sequential(cm))
    cubes = np.zeros((n_frames,) + shape, dtype=np.complex64)
    cubes[:, 0, 0, 0] = np.arange(n_frames)
    mp.load(cubes)
    assert mp.bounds == [shard_bounds(n_frames, r, world) for r in range(world)]
    dets = mp.detect()
    assert [int(d[0, 0]) for d in dets] == list(range(n_frames))
    assert [int(d[0, 1]) for d in dets] == [f * world // n_frames for f in range(n_frames)]
    assert [float(p[0, 0]) for p in mp.point_clouds()] == [float(f) for f in range(n_frames)]
    mp.close()


def test_default_part_factory_hands_sequential_to_every_pipeline(monkeypatch):
    """Without a part_factory the keyword reaches FramePipeline(..., sequential=...) of every device."""
    from mmwave_radar_processing_amd import batch
    cm = make_cm()
    seen = []

    class Part(_FakePart):
        def __init__(self, config_manager, n, shape, ctx=None, **kw):
            super().__init__(ctx, n, shape)
            seen.append(kw)
    monkeypatch.setattr(batch, "FramePipeline", Part)
    monkeypatch.setattr(_lib, "Context", lambda device: device)
    det = sequential(cm)
    mp = MultiDeviceFramePipeline(cm, 8, SHAPE, devices=[0, 1], sequential=det, det_capacity=99)
    assert len(seen) == 2 and all(kw["sequential"] is det and kw["det_capacity"] == 99 for kw in seen)
    mp.parts = []
    for pool in mp._pools:
        pool.shutdown(wait=True)


def test_header_and_ctypes_table_hold_the_revision_7_entries():
    text = open(os.path.join(ROOT, "include", "mmwgpu.h")).read()
    assert int(re.search(r"#define MMWGPU_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 7
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(rf"\bint {name}\s*\(", code), f"{name} is not declared in mmwgpu.h"
        assert name in _lib.EXPORTED and name in _lib._SIGNATURES
    lib = _lib.load_library()
    assert lib.mmw_abi_version() == 7
    # one argtype per parameter of the declaration
    for name in NEW_ENTRIES:
        decl = re.search(rf"\bint {name}\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(_lib._SIGNATURES[name]) == decl.count(",") + 1, name


def test_route_of_shapes_without_a_device():
    """mmw_seq_route reads the shape (and the option of a context; none here): every shipped cfg plane with S <= 3072 is served
    by the row kernel's LDS budget, a plane beyond it takes the full-plane route."""
    lib = _lib.load_library()
    default = lib.mmw_seq_route(None, 256, 128)
    assert default in (0, 1)
    if default == 0:
        for S, C in ((256, 128), (63, 70), (254, 50), (63, 127), (100, 100), (127, 32), (3072, 128), (3072, 8), (64, 512)):
            assert lib.mmw_seq_route(None, S, C) == 0, (S, C)
    assert lib.mmw_seq_route(None, 3072, 2048) == 1
    assert lib.mmw_seq_route(None, 0, 128) == 1
