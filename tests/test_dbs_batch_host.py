"""Host side of FramePipeline.dbs_range_angle: the batched index tables against the per-frame ``_dbs_indices``, the branch a
frame takes at ``min_vel_dbs``, the new C entry in the header and the ctypes table, and the arguments it refuses (no device)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mmwave_radar_processing_amd import _lib, synth
from mmwave_radar_processing_amd.batch import FramePipeline, dbs_branches, dbs_index_tables
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.processors import RangeAngleProcessor, RangeAngleProcessorDBSEnhanced

PER_N_OUT = 2600        # velocities per n_out: 10 400 over the four of them


def make_dbs(n_out=64, **kw):
    cm = ConfigManager()
    cm.load_cfg_text(synth.SYNTH_CFG_256x128x12)
    return RangeAngleProcessorDBSEnhanced(cm, num_angle_bins_dbs_enhanced_response=n_out, **kw)


def midpoint_velocities(dbs, rng, count):
    """Velocities whose Doppler speed at one output angle is, as ``get_dop_vel`` rounds it, EXACTLY the midpoint of two
    neighbouring ``vel_bins`` (found by nudging the speed ulp by ulp), and their neighbours one ulp to either side."""
    ang, bins = dbs.angle_bins_dbs_enhanced, dbs.vel_bins
    exact, near = [], []
    while len(exact) < count:
        i, k = int(rng.integers(len(ang))), int(rng.integers(len(bins) - 1))
        mid = 0.5 * (bins[k] + bins[k + 1])
        m = mid
        for _ in range(4):
            m = np.nextafter(m, -np.inf)
        for _ in range(9):
            v = np.array([-m * np.cos(ang[i]), -m * np.sin(ang[i]), float(rng.normal())])
            if dbs.get_dop_vel(ang[i], v) == mid:
                exact.append(v)
                near += [np.nextafter(v, np.inf), np.nextafter(v, -np.inf)]
                break
            m = np.nextafter(m, np.inf)
    return exact, near


@pytest.mark.parametrize("n_out", [1, 40, 64, 100])
def test_batched_index_tables_equal_the_per_frame_function(n_out):
    """2 600 velocities per n_out (10 400 in all): random ones of either sign, zero, speeds far beyond vel_max (argmin on an
    edge bin), exact midpoints of two Doppler bins and their one-ulp neighbours.  100 > A: several outputs share an angle bin."""
    dbs = make_dbs(n_out)
    assert len(dbs.angle_bins_dbs_enhanced) == n_out
    rng = np.random.default_rng(100 + n_out)
    vmax = dbs.config_manager.vel_max_m_s
    exact, near = midpoint_velocities(dbs, rng, 60)
    special = [np.zeros(3), -np.zeros(3), [1e3 * vmax, 0, 0], [-1e3 * vmax, 0, 0], [0, 50 * vmax, 0], [0, -50 * vmax, -3.0],
               [vmax, vmax, vmax], [-vmax, -vmax, -vmax], [1e300, 1e300, 0], [-4.0, -2.5, -1.0], [-1e-300, -1e-310, 0]]
    # large products that cancel in the Doppler speed of one output angle: the speed is of the order of the bins, its rounding
    # of the order of the products' ulps
    ang = dbs.angle_bins_dbs_enhanced
    for t in (1e3, 1e8, 1e13, -1e15, 1e18):
        i = int(rng.integers(n_out))
        special.append([-t * np.sin(ang[i]) - 0.3 * np.cos(ang[i]), t * np.cos(ang[i]) - 0.3 * np.sin(ang[i]), 1.0])
    v = np.concatenate([np.asarray(special, dtype=np.float64), np.asarray(exact), np.asarray(near)])
    n_rand = PER_N_OUT - len(v)
    v = np.concatenate([v, rng.normal(size=(n_rand // 2, 3)) * vmax / 3, -np.abs(rng.normal(size=(n_rand - n_rand // 2, 3))) * vmax])
    assert v.shape == (PER_N_OUT, 3) and np.all(np.isfinite(v))
    ang_tab, vel_tab = dbs_index_tables(dbs, v)
    assert ang_tab.shape == vel_tab.shape == (PER_N_OUT, n_out) and ang_tab.dtype == vel_tab.dtype == np.int32
    assert ang_tab.flags.c_contiguous and vel_tab.flags.c_contiguous
    edge = 0
    for f in range(PER_N_OUT):
        a, k = dbs._dbs_indices(v[f])
        np.testing.assert_array_equal(ang_tab[f], a, err_msg=f"angle bins of velocity {f}: {v[f]}")
        np.testing.assert_array_equal(vel_tab[f], k, err_msg=f"Doppler bins of velocity {f}: {v[f]}")
        edge += int(np.any(k == 0) or np.any(k == len(dbs.vel_bins) - 1))
    assert edge >= 6                        # the far speeds did reach the edge bins
    if n_out == 100:
        assert len(np.unique(ang_tab[0])) <= dbs.num_angle_bins < n_out


def test_index_tables_of_no_frames_and_of_unsorted_bins():
    dbs = make_dbs(40)
    a, k = dbs_index_tables(dbs, np.zeros((0, 3)))
    assert a.shape == k.shape == (0, 40)
    dbs.vel_bins = dbs.vel_bins[::-1].copy()            # not increasing: every frame goes through _dbs_indices itself
    v = np.random.default_rng(3).normal(size=(20, 3)) * 2
    a, k = dbs_index_tables(dbs, v)
    for f in range(20):
        np.testing.assert_array_equal(k[f], dbs._dbs_indices(v[f])[1])


def test_branch_at_min_vel_dbs():
    """``<`` is false exactly at min_vel_dbs (sharpened); one ulp below it is true (plain range-angle)."""
    dbs = make_dbs(64, min_x_y_vel_dbs=0.25)
    below = np.nextafter(0.25, 0.0)
    v = np.array([[0.25, 0, 0], [below, 0, 9.0], [0, -0.25, 0], [0, -below, 0], [0, 0, 5.0], [0.15, 0.2, 0], [3.0, 4.0, 0]])
    got = dbs_branches(dbs, v)
    assert got.dtype == bool and got.tolist()[:5] == [True, False, True, False, False]
    rng = np.random.default_rng(9)
    phi = rng.uniform(0, 2 * np.pi, 3000)
    speed = 0.25 * (1 + rng.integers(-3, 4, 3000) * 2.0 ** -52)         # within three ulps of the limit, any heading
    w = np.stack([speed * np.cos(phi), speed * np.sin(phi), rng.normal(size=3000)], axis=1)
    w = np.concatenate([v, w, rng.normal(size=(1000, 3)) * 0.3])
    want = np.array([not (np.linalg.norm(x[0:2]) < dbs.min_vel_dbs) for x in w])
    np.testing.assert_array_equal(dbs_branches(dbs, w), want)
    assert 0 < np.count_nonzero(want[7:3007]) < 3000                    # the near-limit set falls on both sides
    np.testing.assert_array_equal(dbs_branches(make_dbs(64, min_x_y_vel_dbs=0.0), np.zeros((2, 3))), [True, True])


def test_header_and_ctypes_table_hold_mmw_dbs_sharpen():
    text = open(os.path.join(ROOT, "include", "mmwgpu.h")).read()
    assert int(re.search(r"#define MMWGPU_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 7
    assert re.search(r"/\*\s*mmw_dbs_sharpen:.*?range_angle_resp_dbs_enhanced\.py:\d+", text, flags=re.S)   # cites the reference
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint mmw_dbs_sharpen\s*\((.*?)\);", code, flags=re.S)
    assert decl, "mmw_dbs_sharpen is not declared in mmwgpu.h"
    assert "mmw_dbs_sharpen" in _lib.EXPORTED
    assert len(_lib._SIGNATURES["mmw_dbs_sharpen"]) == decl.group(1).count(",") + 1 == 14
    lib = _lib.load_library()
    assert lib.mmw_abi_version() == 7 and hasattr(lib, "mmw_dbs_sharpen")


def bare_pipeline(n_frames=3, shape=(12, 256, 128)):
    """A FramePipeline without a device behind it: enough for the checks that come before any buffer is touched."""
    p = FramePipeline.__new__(FramePipeline)
    p.n_frames = n_frames
    p.V, p.S, p.C = shape
    return p


def test_dbs_range_angle_refuses_bad_arguments():
    p = bare_pipeline()
    dbs = make_dbs(64)
    v = np.ones((3, 3))
    cm = dbs.config_manager
    for method in (p.dbs_range_angle, p.dbs_range_angle_device):
        with pytest.raises(ValueError, match="must be a RangeAngleProcessorDBSEnhanced, got RangeAngleProcessor"):
            method(RangeAngleProcessor(cm), v)
        with pytest.raises(ValueError, match="must be a RangeAngleProcessorDBSEnhanced, got object"):
            method(object(), v)
        with pytest.raises(ValueError, match=r"velocities_ned must be \[3, 3\]"):
            method(dbs, np.ones((2, 3)))
        with pytest.raises(ValueError, match=r"velocities_ned must be \[3, 3\]"):
            method(dbs, np.ones(3))
        with pytest.raises(ValueError, match="outside the 12 antennas"):
            method(dbs, v, rx_antennas=[0, 12])
        with pytest.raises(ValueError, match=r"num_angle_bins \(8\) must be >= number of antennas \(12\)"):
            method(RangeAngleProcessorDBSEnhanced(cm, num_angle_bins_range_angle_response=8), v)
        with pytest.raises(ValueError, match=r"num_angle_bins \(8\) must be >= number of antennas \(9\)"):
            method(RangeAngleProcessorDBSEnhanced(cm, num_angle_bins_range_angle_response=8), v, rx_antennas=list(range(9)))
