"""The context's side queues have one owner (mmw_ctx.h: queues_of / drain / drain_all / destroy_queues / create_split_queues):
teardown, scratch regrowth and a new CU split wait for everything that is in flight, whatever queue it is on.  Every case is a
legal use of the API, run once; the results are compared bit for bit (detections, both argmax arrays, spectra)."""
import numpy as np
import pytest

from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.detectors import CaCFAR2D
from test_gpu_parity import _detect_points_raw, _same_points

pytestmark = pytest.mark.gpu
CAP = 512


def _cfar():
    return CaCFAR2D((4, 4), (2, 2), 1e-5)


def _antennas(V):
    return list(range(min(8, V))), list(range(max(0, V - 4), V))


def _synth(ctx, F, shape, seed):
    V, S, C = shape
    d = ctx.alloc(F * V * S * C * 8)
    _lib.check(ctx.lib.mmw_synth_cubes(ctx.handle, d.ptr, F, V, S, C, seed, 8, 30.0))
    return d


def _out_buffers(owner, F, shape):
    """range-Doppler cube, plane norms, detections, counts, azimuth and elevation indices; the last four filled with -7"""
    V, S, C = shape
    b = [owner.alloc(n) for n in (F * V * S * C * 8, F * V * 4, F * CAP * 8, F * 4, F * CAP * 4, F * CAP * 4)]
    for x in b[2:]:
        x.upload(np.full(x.nbytes // 4, -7, np.int32))
    return b


def _deferred_call(ctx, d_in, b, F, shape):
    """one mmw_detect_points call without the statistics: its tail stays on the side queues"""
    V, S, C = shape
    cfar = _cfar()
    az, el = _antennas(V)
    a_az, n_az = _lib.int_array(az)
    a_el, n_el = _lib.int_array(el)
    _lib.check(ctx.lib.mmw_detect_points(ctx.handle, d_in.ptr, b[0].ptr, b[1].ptr, None, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr,
                                         F, V, S, C, cfar.kind, 4, 4, 2, 2, float(cfar._scale()), 0, CAP, a_az, n_az, 1, a_el, n_el,
                                         0, 64, None))


def _result(b, F):
    return (b[3].download((F,), np.int32), b[2].download((F, CAP, 2), np.int32), b[4].download((F, CAP), np.int32),
            b[5].download((F, CAP), np.int32))


def _assert_same(got, ref):
    np.testing.assert_array_equal(got[0], ref[0])
    keep = ref[0] >= 0                  # (a frame the screening hands back has no list to compare)
    _same_points(tuple(x[keep] for x in got), tuple(x[keep] for x in ref[:4]))


@pytest.mark.parametrize("shape,F", [((12, 256, 128), 8), ((12, 63, 100), 16)])
def test_destroy_drains_the_deferred_tail(shape, F):
    """mmw_ctx_destroy straight after a deferred mmw_detect_points call -- no download, no mmw_sync in between -- returns MMW_OK
    and leaves in the caller's buffers (owned by a second context, so they outlive the first) exactly what a call that joins its
    own tail leaves: destroy waits for the tail before it frees the scratch the tail works in.  The band is widened, so the tail
    HAS exact cells and flagged evaluations to do (asserted from the reference's statistics).  256 x 128: the fused kernel;
    63 x 100: a mixed-radix plane."""
    V = shape[0]
    owner, ctx = _lib.Context(0), _lib.Context(0)
    ctx.set_option("MMW_DETECT_BAND_MULT", 20)
    d_in = _synth(owner, F, shape, 515151)
    owner.sync()
    ref = _detect_points_raw(ctx, d_in, F, shape, _cfar(), CAP, *_antennas(V))     # (asks for the statistics: joins its own tail)
    print(f"destroy behind a deferred tail, {shape} x {F}: statistics {ref[4]}")
    assert ref[4][1] > 0 and ref[4][3] + ref[4][4] > 0, ref[4]          # undecided cells and flagged evaluations exist
    b = _out_buffers(owner, F, shape)
    _deferred_call(ctx, d_in, b, F, shape)
    rc = ctx.lib.mmw_ctx_destroy(ctx.handle)
    ctx.handle = None
    assert rc == _lib.MMW_OK
    _assert_same(_result(b, F), ref)
    owner.close()


def test_scratch_regrowth_under_a_pending_tail():
    """A deferred call of 8 frames, at once a deferred call of 64 frames on other inputs into other buffers: the second call's
    scratch (detect_layout: the flagged-evaluation list alone is 2 * n_frames * cap ints, and no region shrinks with n_frames)
    is larger, so ensure_scratch frees the block the first call's pending tail works in -- behind drain_all.  Both results are
    those of calls that join their own tail (taken afterwards: before, they would have grown the scratch already)."""
    shape = (12, 256, 128)
    ctx = _lib.Context(0)
    ctx.set_option("MMW_DETECT_BAND_MULT", 20)
    d_a, d_b = _synth(ctx, 8, shape, 515151), _synth(ctx, 64, shape, 626262)
    b_a, b_b = _out_buffers(ctx, 8, shape), _out_buffers(ctx, 64, shape)
    _deferred_call(ctx, d_a, b_a, 8, shape)
    _deferred_call(ctx, d_b, b_b, 64, shape)
    got_a, got_b = _result(b_a, 8), _result(b_b, 64)
    ref_a = _detect_points_raw(ctx, d_a, 8, shape, _cfar(), CAP, *_antennas(12))
    ref_b = _detect_points_raw(ctx, d_b, 64, shape, _cfar(), CAP, *_antennas(12))
    assert ref_a[4][1] > 0 and ref_a[4][3] + ref_a[4][4] > 0, ref_a[4]  # the pending tail had work in the scratch
    _assert_same(got_a, ref_a)
    _assert_same(got_b, ref_b)
    ctx.close()


def test_recreated_split_queues_leave_results_and_the_chain_alone():
    """MMW_DETECT_SCR_CUS 32 -> 64 -> 32 on one context sends ensure_det_queues through destroy_queues + create_split_queues
    each time: every result is the serial schedule's.  A chain call on the same context afterwards equals the same call on a
    fresh context bit for bit: the detection group's queues and the chain group's do not disturb each other."""
    shape, F = (12, 256, 128), 8
    V, S, C = shape
    ctx = _lib.Context(0)
    d_in = _synth(ctx, F, shape, 9090)
    ctx.set_option("MMW_DETECT_OVERLAP", 0)
    serial = _detect_points_raw(ctx, d_in, F, shape, _cfar(), CAP, *_antennas(V))
    ctx.set_option("MMW_DETECT_OVERLAP", 1)
    for scr_cus in (32, 64, 32):
        ctx.set_option("MMW_DETECT_SCR_CUS", scr_cus)
        got = _detect_points_raw(ctx, d_in, F, shape, _cfar(), CAP, *_antennas(V))
        _assert_same(got[:4], serial)
        assert got[4] == serial[4], (scr_cus, got[4], serial[4])
    cube = d_in.download((F, V, S, C), np.complex64)
    outs = []
    for c in (ctx, _lib.Context(0)):
        d_c, d_out = c.alloc(cube.nbytes), c.alloc(F * 64 * S * C * 8)
        d_c.upload(cube)
        _lib.check(c.lib.mmw_chain3d(c.handle, d_c.ptr, None, d_out.ptr, F, V, S, C, 64, 0))
        outs.append(d_out.download((F, 64, S, C), np.complex64).view(np.uint32))
        c.close()
    np.testing.assert_array_equal(outs[0], outs[1])


def test_destroy_of_a_context_without_side_queues():
    """A context that never created a side queue tears down cleanly (every handle the helpers meet is null): after mmw_sync
    alone, and straight behind a range-Doppler call without a sync -- whose output, in another context's buffer, a new context
    reproduces bit for bit."""
    ctx = _lib.Context(0)
    ctx.sync()
    rc = ctx.lib.mmw_ctx_destroy(ctx.handle)
    ctx.handle = None
    assert rc == _lib.MMW_OK
    shape, F = (12, 64, 32), 2
    V, S, C = shape
    owner = _lib.Context(0)
    d_in = _synth(owner, F, shape, 4242)
    d_out = [owner.alloc(F * V * S * C * 8) for _ in range(2)]
    for d in d_out:
        d.zero()
    owner.sync()
    for i in range(2):
        ctx = _lib.Context(0)
        _lib.check(ctx.lib.mmw_range_doppler(ctx.handle, d_in.ptr, d_out[i].ptr, None, F, V, S, C))
        rc = ctx.lib.mmw_ctx_destroy(ctx.handle)
        ctx.handle = None
        assert rc == _lib.MMW_OK
    got = [d.download((F, V, S, C), np.complex64).view(np.uint32) for d in d_out]
    assert np.any(got[0] != 0)
    np.testing.assert_array_equal(got[0], got[1])
    owner.close()
