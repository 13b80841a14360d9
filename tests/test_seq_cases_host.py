"""The inputs and references of tests/seq_cases.py, checked without a GPU: the Python mirrors of the row kernel's pass size and
LDS need against csrc/mmw_seq.h and include/mmwgpu.h, and the three preconditions test_gpu_seq_edges.py rests on -- the profiles
hold cells that EQUAL their threshold, no case is vacuous, and on the route-agreement scenes no cell of a listed row is close
enough to its threshold for a rounding error of the rows to decide."""
import os
import re

import numpy as np
import pytest

import cfar_cases as cc
import seq_cases as sc
from conftest import ROOT
from mmwave_radar_processing_amd import _lib


def test_pass_rows_and_lds_mirror_the_headers():
    text = open(os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc", "mmw_seq.h")).read()
    assert int(re.search(r"constexpr int SEQ_RPT = (\d+);", text).group(1)) == sc.SEQ_RPT
    assert re.search(r"one pass takes SEQ_RPT \* \(256 / min\(C, 256\)\) selected rows \(8 for C = 128\)", text)
    assert "return SEQ_RPT * (256 / seq_cols(C));" in text and "return C < 256 ? C : 256;" in text
    assert "SEQ_LDS_MAX = 160 * 1024" in text and sc.SEQ_LDS_MAX == 160 * 1024
    assert sc.pass_rows(128) == 8
    want = {128: 8, 100: 8, 50: 20, 127: 8, 3: 340, 1: 1024, 8: 128, 257: 4, 300: 4, 16: 64, 512: 4}
    assert {C: sc.pass_rows(C) for _, _, C in sc.SHAPES} == want
    # include/mmwgpu.h: 16 (S + C) + 25 * 4 * max(C, 256) bytes -- exact where C divides 256 or exceeds it, a ceiling otherwise
    assert "16 (S + C) + 25 * 4 * max(C, 256) bytes of LDS" in open(os.path.join(ROOT, "include", "mmwgpu.h")).read()
    for _, S, C in sc.SHAPES + ((1,) + sc.UNSERVED,):
        doc = 16 * (S + C) + 25 * 4 * max(C, 256)
        assert sc.lds_bytes(S, C) <= doc
        if 256 % C == 0 or C >= 256:
            assert sc.lds_bytes(S, C) == doc
    assert sc.lds_bytes(1024, 512) == 75776 and 64 * 1024 < 75776 <= sc.SEQ_LDS_MAX
    assert sc.lds_bytes(*sc.UNSERVED) == 166784 > sc.SEQ_LDS_MAX
    assert all(sc.lds_bytes(S, C) <= 64 * 1024 for _, S, C in sc.SHAPES if (1, S, C) != sc.BIG_SHAPE)


def test_route_of_the_shapes_without_a_device(monkeypatch):
    monkeypatch.setenv("MMW_SEQ_FULL_PLANE", "0")
    lib = _lib.load_library()
    for _, S, C in sc.SHAPES:
        assert lib.mmw_seq_route(None, S, C) == 0, (S, C)
    assert lib.mmw_seq_route(None, *sc.UNSERVED) == 1


def test_the_new_entry_is_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmwgpu.h")).read(), flags=re.S)
    decl = re.search(r"\bint mmw_cfar1d_rows\s*\((.*?)\);", text, flags=re.S).group(1)
    gated = re.search(r"\bint mmw_cfar1d_gated\s*\((.*?)\);", text, flags=re.S).group(1)
    assert decl.count(",") == gated.count(",") + 1 == len(_lib._SIGNATURES["mmw_cfar1d_rows"]) - 1
    assert "mmw_cfar1d_rows" in _lib.EXPORTED and hasattr(_lib.load_library(), "mmw_cfar1d_rows")
    assert _lib.load_library().mmw_abi_version() == _lib.ABI_VERSION == 7            # an added entry changes no existing signature


# ----------------------------------------------------------------------------------------------------------- mmw_seq_rows
@pytest.mark.parametrize("S", sc.ROWS_S)
def test_profiles_hold_ties_and_no_case_is_vacuous(S):
    """Per case (window, kind, rank, scale) over the four profiles: at scale 1.0 some valid cell equals its threshold, and there
    is a selected and an unselected valid cell -- except where nothing can be selected by construction."""
    n_live = 0
    for T, G, kind, k, scale in sc.rows_cases(S):
        prof = sc.profile_frames(S, T, G)
        assert prof.shape == (4, S)
        thr, mask = sc.rows_reference(prof, kind, T, G, scale, k)
        valid = np.isfinite(thr)
        if sc.rows_case_is_empty(S, T, G, kind):
            assert not mask.any(), (S, T, G, kind)
            continue
        n_valid = S - 2 * (T + G)
        assert valid[1].sum() == n_valid                                   # the constant profile: every valid cell is finite
        if scale == 1.0:
            ties = sum(cc.tie_stats(prof[f], thr[f], mask[f])[0] for f in range(4))
            assert ties >= n_valid > 0, (S, T, G, kind, k)                  # the constant profile alone
            assert not mask[1].any()
            if kind == cc.CA and S >= 255:                                 # the ramp equals the mean of a symmetric window
                assert cc.tie_stats(prof[2], thr[2], mask[2])[0] >= n_valid - 4 * (T + G) - 2
            if kind == cc.OS and S >= 255:
                assert cc.tie_stats(prof[0], thr[0], mask[0])[0] > 0, (S, T, G, k)
        else:
            assert mask[1].sum() == n_valid                                 # one ulp below 1: the whole valid span, a long list
        if n_valid >= 3:
            assert mask.any() and np.any(valid & (mask == 0)), (S, T, G, kind, k, scale)
            n_live += 1
        # the spikes of the edge profile: hits in the first and the last valid cell
        if n_valid >= 2 * (T + G) + 2:
            assert mask[2, T + G] == 1 and mask[2, S - T - G - 1] == 1, (S, T, G, kind, k, scale)
    assert n_live > 0 or S < 5


def test_profiles_of_the_non_finite_frame_hold_a_nan_and_an_infinity():
    for S in sc.ROWS_S[1:]:
        for T, G in sc.rows_windows(S):
            nf = sc.profile_frames(S, T, G)[3]
            assert not np.all(np.isfinite(nf)), (S, T, G)
            if S >= 255:                                 # room for every plant of cfar_cases.nonfinite
                assert np.isnan(nf).any() and np.isinf(nf).any(), (S, T, G)


# ----------------------------------------------------------------------------------------------------------- cubes and lists
@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cubes_and_lists_are_what_the_gpu_test_needs(shape):
    V, S, C = shape
    cubes = sc.cube_batch(shape)
    assert cubes.shape == (sc.N_FRAMES, V, S, C) and cubes.dtype == np.complex64
    assert np.all(cubes.real == np.round(cubes.real)) and np.all(cubes.imag == np.round(cubes.imag))
    if V > 1:
        assert not np.array_equal(cubes[:, 0], cubes[:, 1])
    assert not np.array_equal(cubes[0], cubes[1])
    rb = sc.pass_rows(C)
    lists = sc.shape_lists(shape)
    assert [len(x) for x in lists[:3]] == [0, 1, 1] and lists[1][0] == 0 and lists[2][0] == S - 1
    assert len(lists) == sc.N_FRAMES and len(lists[5]) == min(rb + 1, S)
    if shape == sc.BIG_SHAPE:
        assert max(len(x) for x in lists + sc.pass_lists(shape)) <= sc.MAX_BIG_ROWS
    else:
        assert len(lists[3]) == S and lists[4].tolist() == list(range(1, S, 2))
        assert [len(x) for x in sc.pass_lists(shape)] == [n for n in (rb - 1, rb, 2 * rb) if 0 < n <= S]
    for lst in lists + sc.pass_lists(shape):
        assert np.all(np.diff(lst) > 0) and (len(lst) == 0 or (lst[0] >= 0 and lst[-1] < S))
    # tone rows fall inside and outside the lists
    tone_rows = {r for f in range(sc.N_FRAMES) for r, _, _ in sc.tones(shape, f)}
    if S >= 8:
        for lst in lists[1:3] + lists[4:]:
            assert len(lst) == S or tone_rows - set(lst.tolist()), (shape, lst)
        assert tone_rows & set(lists[4].tolist()) and tone_rows & set(lists[5].tolist())
    rows, nrows = sc.pack_lists(lists, S)
    assert rows.shape == (6, S) and nrows.tolist() == [len(x) for x in lists]
    assert np.all(rows[0] == sc.ROW_POISON) and rows[1, 0] == 0 and np.all(rows[1, 1:] == sc.ROW_POISON)


@pytest.mark.parametrize("shape", sc.ROUTE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_margin_of_the_route_agreement_scenes(shape):
    """No valid cell of a listed oracle row within 10 x the value bound x (1 + scale) of its threshold: both routes, whose rows
    are within the bound of the oracle's, must then decide as the oracle does.  And the scenes are not empty."""
    cubes, lists = sc.cube_batch(shape), sc.shape_lists(shape)
    n_dets = 0
    for T, G in sc.DET_WINDOWS:
        for kind, k in sc.det_kinds(T):
            for f, lst in enumerate(lists):
                assert sc.margin_violations(cubes[f], lst, kind, T, G, sc.DET_SCALE, k) == 0, (shape, T, G, kind, f)
                plane = sc.oracle_plane(cubes[f])
                n_dets += len(sc.expected_dets(lst, plane[lst], kind, T, G, sc.DET_SCALE, k)[0])
    assert n_dets > 50
    assert 0 < sc.value_bound(cubes[0]) < 1e-6 * sc.oracle_plane(cubes[0]).max()


def test_expected_dets_order_and_close_count():
    x = np.array([[1.0, 1.0, 9.0, 1.0, 1.0, 1.0, 8.0], [5.0, 1.0, 1.0, 1.0, 1.0, 7.0, 1.0]])
    pairs, close = sc.expected_dets([4, 2], x, cc.CA, 1, 0, 2.0)
    assert pairs.tolist() == [[4, 2], [2, 5]] and pairs.dtype == np.int32
    assert close == 0
    x[0, 2] = 2.0                                      # exactly scale * mean(1, 1)
    pairs, close = sc.expected_dets([4, 2], x, cc.CA, 1, 0, 2.0)
    assert pairs.tolist() == [[2, 5]] and close == 1
    assert sc.expected_dets([], x[:0], cc.CA, 1, 0, 2.0)[0].shape == (0, 2)


# ----------------------------------------------------------------------------------------------------------- mmw_cfar1d_rows
@pytest.mark.parametrize("shape", sc.PLANE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_planes_for_the_list_search_hold_ties_and_hits(shape):
    R, D = shape
    lists = sc.plane_lists(R)
    assert [len(x) for x in lists] == [0, 1, 1, R, (R + 1) // 2, 2]
    assert (R * D % 256 == 0) == (shape == (32, 72))
    T, G = sc.PLANE_WINDOW
    planes = sc.planes_for_lists(shape)
    for kind in (cc.CA, cc.OS, cc.GO, cc.SO):
        mask = sc.plane_reference(planes["quantised"], lists, kind)
        assert not mask[0].any() and mask[3].sum() > 8 and mask[1, 1:].sum() == 0
        ties = sum(cc.tie_stats(planes["quantised"][3, r], sc.ref1d(planes["quantised"][3, r], kind, T, G, 1.0, 4)[0],
                                mask[3, r])[0] for r in range(R))
        assert ties > 0, (shape, kind)
        assert not sc.plane_reference(planes["constant"], lists, kind).any()
        assert sc.plane_reference(planes["constant"], lists, kind, cc.JUST_BELOW_ONE)[3].sum() == R * (D - 2 * (T + G))
        assert sc.plane_reference(planes["nonfinite"], lists, kind)[3].sum() > 0
