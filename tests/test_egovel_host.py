"""Host side of the batched ego velocity: the mirrored VelocityEstimator against the reference's recorded results, the table
builders against the recorded draws, the state scan over joined shards, the ABI additions, and the import without scikit-learn."""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT
from egovel_cases import DEGENERATE, Geometry, cases, rel_err
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import MultiDeviceFramePipeline, ego_state_scan, shard_bounds
from mmwave_radar_processing_amd.point_cloud_processing import VelocityEstimator, ransac_tables as T
from mmwave_radar_processing_amd.point_cloud_processing.vel_estimator import ransac_fit

NEW_ENTRIES = ("mmw_point_cloud", "mmw_ego_velocity_ransac")
GEOMETRY = {2: "standard", 3: "ods"}


def fit_of(est, dim, pts):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return (est.lsq_fit_ego_vel_ransac_points_2D if dim == 2 else est.lsq_fit_ego_vel_ransac_points_3D)(points=pts)


@pytest.mark.parametrize("dim", [2, 3])
def test_mirrored_fits_equal_the_reference_frame_by_frame(dim):
    pytest.importorskip("sklearn")
    c = cases()
    est = VelocityEstimator(Geometry(GEOMETRY[dim]))
    want = c.fits[dim]
    for i, (name, pts) in enumerate(zip(c.names, c.points)):
        got = fit_of(est, dim, pts)
        if len(pts) == 0:                       # the reference's own asymmetry: a bare vector in 2-D, a triple in 3-D
            if dim == 2:
                assert isinstance(got, np.ndarray) and got.tolist() == [0.0, 0.0]
            else:
                assert got[0].tolist() == [0.0, 0.0, 0.0] and got[1:] == (0.0, 0.0)
            continue
        coef, r2, share = got
        failed = want["share"][i] == 0.0
        if failed:                              # N = 9, every trial skipped, a non-finite H: zeros, a 2-vector in 3-D too
            assert name in ("clean_9", "no_inlier", "range_zero"), name
            assert coef.shape == (2,) and coef.tolist() == [0.0, 0.0] and (r2, share) == (0.0, 0.0)
            continue
        assert coef.shape == (dim,)
        np.testing.assert_allclose(coef, want["coef"][i][:dim], rtol=1e-12, atol=1e-13, err_msg=name)
        np.testing.assert_allclose([r2, share], [want["r2"][i], want["share"][i]], rtol=1e-12, atol=1e-13, err_msg=name)
        mask = ransac_fit(pts, dim, return_mask=True)[3]
        np.testing.assert_array_equal(mask, want["mask"][i], err_msg=name)
    assert {"clean_9", "no_inlier"} <= set(c.names) and set(DEGENERATE) <= set(c.names)


@pytest.mark.parametrize("geometry", ["standard", "ods"])
def test_process_loop_equals_the_reference_track_and_keeps_stale_statistics(geometry):
    pytest.importorskip("sklearn")
    c = cases()
    est = VelocityEstimator(Geometry(geometry))
    assert est.current_velocity_estimate.tolist() == [0.0, 0.0, 0.0] and est.proposed_velocity_estimate.shape == (0,)
    assert (est.min_R2_threshold, est.min_inlier_percent, est.estimated_R2, est.inlier_percent) == (0.6, 0.75, 0.0, 0.0)
    empties = 0
    for f, pts in enumerate(c.seq):
        before = (est.estimated_R2, est.inlier_percent, est.proposed_velocity_estimate)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = est.process(points=pts if f % 2 else pts.tolist())       # lists are taken too
        assert rel_err(out, c.track[geometry][f]) <= 1e-12, f
        np.testing.assert_allclose([est.estimated_R2, est.inlier_percent], c.stats[geometry][f], rtol=1e-12, atol=1e-13)
        if len(pts) == 0:
            empties += 1
            assert (est.estimated_R2, est.inlier_percent) == before[:2] and est.proposed_velocity_estimate is before[2]
        est.update_history(estimated=out)
    assert empties >= 3 and len(est.history_R2_statistics) == len(est.history_inlier_statistics) == len(c.seq)
    assert len(est.history_estimated) == len(c.seq)
    est.reset()
    assert est.history_R2_statistics == [] and est.history_inlier_statistics == [] and est.history_estimated == []
    # the track holds its value over frames whose fit is not adopted, and moves otherwise
    track = c.track[geometry]
    assert np.any(np.all(track[1:] == track[:-1], axis=1)) and np.any(np.any(track[1:] != track[:-1], axis=1))


def test_table_builders_equal_the_recorded_draws():
    pytest.importorskip("sklearn")
    c = cases()
    assert {10, 11, 64, 65, 256, 257, c.cap} <= set(c.table_n.tolist())
    for n, sub, trials in zip(c.table_n.tolist(), c.table_subsets, c.table_trials):
        np.testing.assert_array_equal(T.subset_table(n), sub)
        np.testing.assert_array_equal(T.trials_table(n), trials)
        np.testing.assert_array_equal(T.trials_table_full(n), trials)
        assert trials[n] == 1 and trials[0] == 20 and np.all(np.diff(trials) <= 0)
    assert T.subset_table(10)[0].tolist() == list(range(10))             # every subset of 10 points is the whole set
    counts = np.concatenate([c.counts, c.seq_counts])
    got, want = T.frame_tables(counts), c.tables_for(counts)
    for f, n in enumerate(counts):
        if n < 10:
            assert got[1][f] == -1
            continue
        r, w = got[1][f], want[1][f]
        np.testing.assert_array_equal(got[0][r], want[0][w])
        np.testing.assert_array_equal(got[2][got[3][r]:got[3][r] + n + 1], want[2][want[3][w]:want[3][w] + n + 1])
    with pytest.raises(ValueError):
        T.subset_table(9)
    with pytest.raises(ValueError):
        T.seed_tables(12, c.table_subsets[0], c.table_trials[0])


class _FitPart:
    """A device's share of a batch whose fits are already known."""

    def __init__(self, fits, counts):
        self.fits, self.counts, self.lo, self.n, self.n_ego_flagged = fits, counts, 0, 0, 1

    def ego_fits(self, estimator):
        return self.fits[self.lo:self.lo + self.n], self.counts[self.lo:self.lo + self.n]


@pytest.mark.parametrize("geometry,dim", [("standard", 2), ("ods", 3)])
def test_state_scan_over_joined_shards_equals_the_track(geometry, dim):
    pytest.importorskip("sklearn")
    c = cases()
    fits = np.zeros((len(c.seq), dim + 2))
    for f, pts in enumerate(c.seq):
        if len(pts):
            coef, r2, share = fit_of(VelocityEstimator(Geometry(geometry)), dim, pts)
            fits[f, :len(coef)], fits[f, dim:] = coef, (r2, share)
    one = ego_state_scan(VelocityEstimator(Geometry(geometry)), fits, c.seq_counts)
    assert one.shape == (len(c.seq), 3) and rel_err(one, c.track[geometry]) <= 1e-12
    est = VelocityEstimator(Geometry(geometry))                            # two calls of 20: the state carries
    two = np.concatenate([ego_state_scan(est, fits[:20], c.seq_counts[:20]), ego_state_scan(est, fits[20:], c.seq_counts[20:])])
    np.testing.assert_array_equal(one, two)
    world, F = 3, len(c.seq)
    mp = MultiDeviceFramePipeline(None, max_frames=F, shape=(2, 2, 2), devices=list(range(world)),
                                  part_factory=lambda d, n: _FitPart(fits, c.seq_counts))
    mp._set_frames(F)
    for r, part in enumerate(mp.parts):
        part.lo, part.n = shard_bounds(F, r, world)[0], shard_bounds(F, r, world)[1] - shard_bounds(F, r, world)[0]
    np.testing.assert_array_equal(mp.ego_velocities(VelocityEstimator(Geometry(geometry))), one)
    assert mp.n_ego_flagged == world
    mp.parts = []
    for pool in mp._pools:
        pool.shutdown(wait=True)


def test_header_ctypes_table_and_makefile_list_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "mmwgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load_library()
    for name in NEW_ENTRIES:
        decl = re.search(rf"\bint {name}\s*\((.*?)\);", code, flags=re.S)
        assert decl, f"{name} is not declared in mmwgpu.h"
        assert name in _lib.EXPORTED and len(_lib._SIGNATURES[name]) == decl.group(1).count(",") + 1
        assert hasattr(lib, name)
    assert lib.mmw_abi_version() == _lib.ABI_VERSION == 7
    make = open(os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS = .*\bmmw_tu_egovel\b", make, flags=re.M)
    assert re.search(r"^build/mmw_tu_egovel\.o:.*-ffp-contract=off", make, flags=re.M)
    assert os.path.exists(os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc", "mmw_tu_egovel.hip"))
    # argument checks that need no device
    assert lib.mmw_ego_velocity_ransac(None, None, None, 0, 1, 2, 0.15, 0.6, None, None, 0, None, 0, None, None, None, None) == -1
    assert lib.mmw_point_cloud(None, None, None, None, None, None, None, None, None, None, 0, 1, 1, 1, 1) == -1


def test_package_imports_without_scikit_learn():
    code = ("import sys; sys.modules['sklearn'] = None\n"
            "import mmwave_radar_processing_amd, mmwave_radar_processing_amd.batch\n"
            "from mmwave_radar_processing_amd.point_cloud_processing import VelocityEstimator, ransac_tables\n"
            "import numpy as np\n"
            "assert ransac_tables.trials_table(12)[12] == 1\n"
            "try:\n    ransac_tables.subset_table(12)\nexcept ImportError as e:\n    print('lazy:', e)\nelse:\n    raise SystemExit('sklearn was importable')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "lazy:" in out.stdout, out.stderr[-2000:]
