"""Device-resident multi-frame pipeline and per-frame sharding across GPUs.

The reference processes frames one by one in a Python loop (scripts/test_vel_estimation.py:145-151,
plotting/movie_generator.py:138-150).  Frames are independent for every processor on the hot path
(SURVEY.md section 8e), so a batch is processed as ``[F, V, S, C]`` cubes resident in HBM, and a multi-GPU job
is a contiguous block split of the frame range -- one process per GPU, NO collective on the data path; only
the host-side join of per-frame results (``gather_frames``) touches ``torch.distributed``.
"""
from __future__ import annotations

import ctypes
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .detectors.base import BaseCFAR1D
from .detectors.ca_cfar import CaCFAR2D
from .processors.range_angle_resp import angle_tables
from .processors.steering_beamformers import (CAPON_PASS_BUDGET, CAPON_POINTS_PASS_FRAMES, array_pattern_args,  # noqa: F401
                                              array_patterns, array_patterns_on, capon_cube_args, capon_doppler_on,
                                              capon_from_cubes, capon_pass_frames, capon_passes, capon_points_args)


def shard_bounds(n_frames: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous block split: frame f belongs to rank floor(f * world / n_frames)."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError(f"bad rank/world {rank}/{world}")
    lo = -(-rank * n_frames // world)           # ceil(rank * F / world)
    hi = -(-(rank + 1) * n_frames // world)
    return lo, hi


def gather_frames(local: Sequence, n_frames: int, dist=None) -> Optional[List]:
    """Join per-frame results (one picklable object per local frame) on rank 0 in global frame order.

    ``dist`` is an initialised ``torch.distributed`` module (any backend with object collectives, e.g. gloo)
    or None for a single process.  Returns the list on rank 0, None elsewhere."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        if len(local) != n_frames:
            raise ValueError("single-process gather needs all frames")
        return list(local)
    world, rank = dist.get_world_size(), dist.get_rank()
    lo, hi = shard_bounds(n_frames, rank, world)
    if len(local) != hi - lo:
        raise ValueError(f"rank {rank} holds {len(local)} frames, expected {hi - lo}")
    parts = [None] * world if rank == 0 else None
    dist.gather_object(list(local), parts, dst=0)
    if rank != 0:
        return None
    out: List = []
    for p in parts:
        out.extend(p)
    return out


def run_sharded(process_range: Callable[[int, int], Sequence], n_frames: int, dist=None) -> Optional[List]:
    """``process_range(lo, hi)`` -> per-frame results of this rank's block; joined on rank 0."""
    if dist is None or not dist.is_initialized():
        return list(process_range(0, n_frames))
    lo, hi = shard_bounds(n_frames, dist.get_rank(), dist.get_world_size())
    return gather_frames(process_range(lo, hi), n_frames, dist)


def _check_stock_cfar1d(kw: str, role: str, det) -> None:
    """A batched path runs ``det`` through ``cfar1d_threshold`` on the device, so it must be one of the stock 1-D CFARs."""
    if not isinstance(det, BaseCFAR1D):
        raise ValueError(f"{kw}=: the {role} detector {type(det).__name__} is not a 1-D CFAR (a 2-D registry key); "
                         f"the batched {kw} path runs the stock 1-D detectors only -- use the per-frame API")
    if type(det)._compute_thresholds is not BaseCFAR1D._compute_thresholds or \
            det.kind not in (_lib.CFAR_CA, _lib.CFAR_OS, _lib.CFAR_GO, _lib.CFAR_SO):
        raise ValueError(f"{kw}=: the {role} detector {type(det).__name__} computes its own thresholds; the batched "
                         f"{kw} path runs the stock CA / OS / GO / SO 1-D detectors only -- use the per-frame API")


def _check_ground(ground, shape: Tuple[int, int, int]) -> None:
    """What the batched ground path serves: a RangeDopplerGroundDetector whose velocity detector is a stock 1-D CFAR."""
    from .processors.range_doppler_detection.range_doppler_ground_detector import RangeDopplerGroundDetector
    if not isinstance(ground, RangeDopplerGroundDetector):
        raise ValueError(f"ground= takes a RangeDopplerGroundDetector, got {type(ground).__name__}")
    _check_stock_cfar1d("ground", "velocity", ground.vel_detector)
    S = shape[1]
    if len(ground.altimeter.range_bins) != S or len(ground.range_bins) != S:
        raise ValueError(f"ground=: the detector's range tables do not have {S} bins (config and cube shape disagree)")


def _check_integrate_rx(integrate_rx, V: int) -> List[int]:
    """The antenna list of ``FramePipeline(integrate_rx=...)``: non-empty, ints in ``[0, V)``, each listed once."""
    try:
        items = list(integrate_rx)
    except TypeError:
        raise ValueError(f"integrate_rx= takes a list of antenna indices, got {type(integrate_rx).__name__}") from None
    if not items:
        raise ValueError("integrate_rx= must list at least one antenna")
    for v in items:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"integrate_rx= takes ints, got {v!r}")
        if not 0 <= int(v) < V:
            raise ValueError(f"integrate_rx=: antenna {int(v)} is outside [0, {V})")
    ants = [int(v) for v in items]
    if len(set(ants)) != len(ants):
        raise ValueError(f"integrate_rx=: an antenna is listed twice in {ants}")
    if len(ants) > 32:
        raise ValueError("integrate_rx=: at most 32 antennas")
    return ants


def tdm_tx_slots_of(tdm_tx_slots, V: int, num_rx: int) -> Tuple[List[int], int]:
    """The transmit slot of every virtual antenna and the number of slots in a loop, for ``tdm_compensation=True``.  ``None``:
    ``slot[v] = v // num_rx`` and ``V // num_rx`` slots (the order VirtualArrayReformatter stacks the antennas in).  A list: one
    non-negative int per virtual antenna; the loop has ``max(slot) + 1`` slots."""
    if tdm_tx_slots is None:
        num_rx = int(num_rx)
        if num_rx < 1 or V % num_rx:
            raise ValueError(f"tdm_compensation: {V} virtual antennas are no multiple of num_rx_antennas = {num_rx}; pass tdm_tx_slots=")
        return [v // num_rx for v in range(V)], V // num_rx
    try:
        items = list(tdm_tx_slots)
    except TypeError:
        raise ValueError(f"tdm_tx_slots= takes a list of ints, got {type(tdm_tx_slots).__name__}") from None
    if len(items) != V:
        raise ValueError(f"tdm_tx_slots= needs one slot per virtual antenna ({V}), got {len(items)}")
    for v in items:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"tdm_tx_slots= takes ints, got {v!r}")
        if int(v) < 0:
            raise ValueError(f"tdm_tx_slots=: slot {int(v)} is negative")
    slots = [int(v) for v in items]
    return slots, max(slots) + 1


def tdm_phase_table(ant, slots, n_slots: int, C: int) -> np.ndarray:
    """The factors of the TDM-MIMO Doppler phase compensation, complex128 ``[len(ant), C]``:
    ``p[i][c] = exp(-2 pi j slots[ant[i]] (c - C // 2) / (n_slots C))`` for the fftshifted Doppler column ``c``.  Made once on the
    host in float64; the kernels, the host twin and the tests' NumPy restatement all multiply by these very values."""
    ant = np.asarray(ant, dtype=np.int64).reshape(-1)
    slots = np.asarray(slots, dtype=np.int64).reshape(-1)
    n_slots, C = int(n_slots), int(C)
    if n_slots < 1 or C < 1:
        raise ValueError("tdm_phase_table: n_slots and C must be positive")
    if ant.size and (ant.min() < -slots.size or ant.max() >= slots.size):
        raise ValueError("tdm_phase_table: antenna index outside the slot list")
    k = slots[ant].astype(np.float64)[:, None]
    col = (np.arange(C, dtype=np.int64) - C // 2).astype(np.float64)[None, :]
    ang = -2.0 * np.pi * (k * col) / float(n_slots * C)
    return np.ascontiguousarray(np.cos(ang) + 1j * np.sin(ang), dtype=np.complex128)


def tdm_unwrapped_bin(c, h, n_slots: int, C: int):
    """The Doppler bin of fftshifted column ``c`` under velocity hypothesis ``h``: ``k' = sym(k + h C)`` with
    ``k = c - C // 2``, ``M = n_slots C`` and ``sym(q) = ((q + M // 2) mod M) - M // 2`` (integers, floor mod).  Scalars or arrays;
    ``m = (k' - k) / C`` is exact, and ``|m| <= (n_slots + 1) // 2``."""
    n_slots, C = int(n_slots), int(C)
    if n_slots < 1 or C < 1:
        raise ValueError("tdm_unwrapped_bin: n_slots and C must be positive")
    M = n_slots * C
    q = (np.asarray(c, dtype=np.int64) - C // 2) + np.asarray(h, dtype=np.int64) * C
    out = ((q + M // 2) % M) - M // 2
    return int(out) if out.ndim == 0 else out


def tdm_hypothesis_table(ant, slots, n_slots: int, C: int) -> np.ndarray:
    """The factors of every velocity hypothesis of a TDM-MIMO detection, complex128 ``[n_slots, len(ant), C]``:
    ``p_h[i][c] = exp(-2 pi j q / M)`` with ``q = sym(slots[ant[i]] (k + h C))``, ``k = c - C // 2``, ``M = n_slots C`` -- the phase
    is reduced as an int64 before it becomes a float, so hypotheses the list cannot tell apart are equal bit for bit, and
    ``table[0]`` is ``tdm_phase_table(ant, slots, n_slots, C)`` bit for bit (``|slot k| < M / 2``: the reduction leaves it alone)."""
    ant = np.asarray(ant, dtype=np.int64).reshape(-1)
    slots = np.asarray(slots, dtype=np.int64).reshape(-1)
    n_slots, C = int(n_slots), int(C)
    if n_slots < 1 or C < 1:
        raise ValueError("tdm_hypothesis_table: n_slots and C must be positive")
    if ant.size and (ant.min() < -slots.size or ant.max() >= slots.size):
        raise ValueError("tdm_hypothesis_table: antenna index outside the slot list")
    M = n_slots * C
    k = (np.arange(C, dtype=np.int64) - C // 2)[None, None, :]
    h = np.arange(n_slots, dtype=np.int64)[:, None, None]
    q = slots[ant][None, :, None] * (k + h * C)
    q = ((q + M // 2) % M) - M // 2
    ang = -2.0 * np.pi * q.astype(np.float64) / float(M)
    return np.ascontiguousarray(np.cos(ang) + 1j * np.sin(ang), dtype=np.complex128)


def tdm_hypothesis_list_of(tdm_hypothesis_list, az, el, tdm_slots) -> Tuple[str, List[int]]:
    """The list whose angle peak decides the velocity hypothesis, for ``tdm_velocity_unwrap=True``: ``("az" | "el" | "list",
    antennas)``.  ``"az"`` / ``"el"``: the pipeline's own list; else distinct ints.  A list inside one transmit slot is refused (its
    hypotheses differ by a common phase: it carries no information), and so are more than 8 slots.  Whether the list is a
    UNIFORM aperture -- which the decision needs -- cannot be checked here."""
    slots, n_slots = tdm_slots
    if isinstance(tdm_hypothesis_list, str):
        if tdm_hypothesis_list not in ("az", "el"):
            raise ValueError(f"tdm_hypothesis_list= takes 'az', 'el' or a list of antennas, got {tdm_hypothesis_list!r}")
        which, ants = tdm_hypothesis_list, list(az if tdm_hypothesis_list == "az" else el)
    else:
        try:
            items = list(tdm_hypothesis_list)
        except TypeError:
            raise ValueError(f"tdm_hypothesis_list= takes 'az', 'el' or a list of antennas, got "
                             f"{type(tdm_hypothesis_list).__name__}") from None
        for v in items:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -len(slots) <= int(v) < len(slots):
                raise ValueError(f"tdm_hypothesis_list=: {v!r} is no antenna index of {len(slots)} virtual antennas")
        which, ants = "list", [int(v) for v in items]
        if len(set(a % len(slots) for a in ants)) != len(ants) or len(ants) > 32:
            raise ValueError(f"tdm_hypothesis_list=: up to 32 distinct antennas, got {ants}")
    if n_slots > 8:
        raise ValueError(f"tdm_velocity_unwrap: {n_slots} transmit slots, at most 8 hypotheses are evaluated")
    if len(set(slots[a] for a in ants)) < 2:
        raise ValueError(f"tdm_velocity_unwrap: the deciding list {ants} lies inside one transmit slot and carries no information "
                         "about the velocity hypothesis; pass tdm_hypothesis_list=")
    return which, ants


def tdm_distinct_hypotheses(table: np.ndarray) -> List[int]:
    """For every hypothesis of a ``[H, n_ant, C]`` table the number of the hypothesis that stands for it: itself,
    or the first earlier one whose block is equal bit for bit or is, like its own, a phase common to the whole list (all rows
    equal bit for bit -- no magnitude can tell two of those apart).  The rule the library applies with ``memcmp``."""
    t = np.ascontiguousarray(table, dtype=np.complex128)
    common = [all(t[h, i].tobytes() == t[h, 0].tobytes() for i in range(t.shape[1])) for h in range(t.shape[0])]
    out: List[int] = []
    for h in range(t.shape[0]):
        rep = h
        for g in range(h):
            if out[g] == g and ((common[h] and common[g]) or t[h].tobytes() == t[g].tobytes()):
                rep = g
                break
        out.append(rep)
    return out


def _check_sequential(sequential) -> None:
    """What the batched sequential path serves: a RangeDopplerDetectorSequential whose two detectors are stock 1-D CFARs."""
    from .processors.range_doppler_detection.range_doppler_detector_sequential import RangeDopplerDetectorSequential
    if not isinstance(sequential, RangeDopplerDetectorSequential):
        raise ValueError(f"sequential= takes a RangeDopplerDetectorSequential, got {type(sequential).__name__}")
    _check_stock_cfar1d("sequential", "range", sequential.rng_detector)
    _check_stock_cfar1d("sequential", "velocity", sequential.vel_detector)


def _cfar1d_args(det) -> Tuple[int, int, int, float, int]:
    return int(det.kind), int(det.num_train), int(det.num_guard), float(det._scale()), int(det._k_rank())


def ground_gates(range_bins: np.ndarray, altitudes_m: np.ndarray) -> np.ndarray:
    """``slant_gate`` (range_doppler_ground_detector.py) for every frame at once: int32 ``[F, 2]`` rows (near, far), both
    included; far < near is an empty gate.  The same float64 operations as the per-frame function, vectorised."""
    alt = np.asarray(altitudes_m, dtype=np.float64)
    far_m = np.minimum(range_bins[-1], alt / np.cos(np.deg2rad(60.0)))
    near = np.abs(range_bins[None, :] - alt[:, None]).argmin(axis=1)
    far = np.abs(range_bins[None, :] - far_m[:, None]).argmin(axis=1)
    return np.ascontiguousarray(np.stack([near, far], axis=1), dtype=np.int32)


DBS_TIE_MARGIN = 1e-9      # relative margin below which a batched nearest-bin / branch decision is re-made by the per-frame code


def dbs_index_tables(dbs, velocities_ned: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``dbs._dbs_indices(v)`` of every row ``v`` of ``velocities_ned`` at once: two int32 ``[F, n_out]`` tables (angle bin,
    Doppler bin), identical to the per-frame function entry by entry.

    The per-frame function takes ``np.dot`` of a normalised 3-vector per output angle and an argmin over ``vel_bins``
    (reference: range_angle_resp_dbs_enhanced.py:200-214,239-255).  The batched restatement (one matrix product, a
    ``searchsorted`` between the two neighbouring bins) may round a Doppler speed differently by a few ulps, which can only
    change the answer where the speed sits within those ulps of the midpoint of two bins.  So every frame holding an entry whose
    two candidate distances differ by less than ``DBS_TIE_MARGIN`` of the scale of the products summed into the speed (and of the
    bins) -- seven decades above the rounding, however far the products cancel --
    or that is not finite, is handed to ``_dbs_indices`` itself; so is everything when ``vel_bins`` is not strictly
    increasing or holds fewer than two bins.  tests/test_dbs_batch_host.py holds the identity on midpoint, edge and random velocities."""
    v = np.asarray(velocities_ned, dtype=np.float64).reshape(-1, 3)
    ang = np.asarray(dbs.angle_bins_dbs_enhanced, dtype=np.float64)
    bins = np.asarray(dbs.vel_bins, dtype=np.float64)
    F, n_out = v.shape[0], ang.shape[0]
    ang_row = np.argmin(np.abs(np.asarray(dbs.angle_bins_no_dbs_enhancement)[None, :] - ang[:, None]), axis=1)
    ang_tab = np.ascontiguousarray(np.broadcast_to(ang_row.astype(np.int32), (F, n_out)))
    vel_tab = np.zeros((F, n_out), dtype=np.int32)
    if F == 0 or n_out == 0:
        return ang_tab, vel_tab
    if bins.size >= 2 and np.all(np.diff(bins) > 0):
        r = np.stack([np.cos(ang), np.sin(ang), np.zeros_like(ang)], axis=1)
        r = r / np.linalg.norm(r, axis=1, keepdims=True)
        with np.errstate(invalid="ignore", over="ignore"):
            dop = -(v @ r.T)                                               # [F, n_out]
            hi = np.clip(np.searchsorted(bins, dop), 1, bins.size - 1)     # the two neighbours; bins 0, 1 / the last two
            lo = hi - 1                                                    # beyond either end
            d_lo, d_hi = np.abs(bins[lo] - dop), np.abs(bins[hi] - dop)
            vel_tab[:] = np.where(d_lo <= d_hi, lo, hi)                    # argmin keeps the first of two equal distances
            # the two roundings of a speed differ by ulps of its TERMS (|v_x cos| + |v_y sin|), which cancel in the speed itself
            scale = np.maximum(np.max(np.abs(bins)), np.abs(v) @ np.abs(r.T))
            sure = np.abs(d_lo - d_hi) > DBS_TIE_MARGIN * scale            # false for NaN
        redo = np.flatnonzero(~np.all(sure, axis=1))
    else:
        redo = np.arange(F)
    for f in redo:
        vel_tab[f] = dbs._dbs_indices(v[f])[1]
    return ang_tab, vel_tab


def dbs_branches(dbs, velocities_ned: np.ndarray) -> np.ndarray:
    """bool ``[F]``: the frames ``dbs.process`` sharpens, i.e. NOT ``np.linalg.norm(v[0:2]) < dbs.min_vel_dbs``
    (range_angle_resp_dbs_enhanced.py:329).  Speeds within ``DBS_TIE_MARGIN`` of the limit, and non-finite ones, are decided by
    that very expression frame by frame."""
    v = np.asarray(velocities_ned, dtype=np.float64).reshape(-1, 3)
    lim = float(dbs.min_vel_dbs)
    with np.errstate(invalid="ignore", over="ignore"):
        speed = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])
        sharp = ~(speed < lim)
        sure = np.abs(speed - lim) > DBS_TIE_MARGIN * max(abs(lim), np.finfo(np.float64).tiny)
    for f in np.flatnonzero(~sure):
        sharp[f] = not (np.linalg.norm(v[f][0:2]) < lim)
    return sharp


def micro_doppler_history(rows: np.ndarray, num_frames_history: int) -> np.ndarray:
    """The ``(C, H)`` spectrogram a ``MicroDopplerProcessor(num_frames_history=H)`` holds after stepping, from a reset, through the
    frames whose rows are ``rows`` (``[n, C]``, oldest first -- ``FramePipeline.micro_doppler``'s output, or the concatenation of
    it over ``stream()`` chunks): the newest row in column 0, zeros behind the frames seen."""
    rows = np.asarray(rows, dtype=np.float64)
    H = int(num_frames_history)
    if rows.ndim != 2 or H < 0:
        raise ValueError(f"micro_doppler_history: rows must be [n_frames, C] and num_frames_history >= 0, got {rows.shape}, {H}")
    out = np.zeros((rows.shape[1], H))
    kept = min(H, rows.shape[0])
    if kept:
        out[:, :kept] = rows[::-1][:kept].T
    return out


def synthetic_array_geometry(proc, velocities) -> Tuple[np.ndarray, np.ndarray]:
    """``(valid, P)``: what a freshly configured ``SyntheticArrayBeamformerProcessor`` like ``proc`` would hold in
    ``array_geometry_valid`` / ``array_geometry`` after each of the frames whose velocities are ``velocities [n, 3]`` -- ``valid``
    bool ``[n]``, ``P`` float64 ``[n_valid, 3, E]`` (``E = num_frames * Cv``, oldest frame of the window first: the layout
    ``mmw_synth_array`` and ``SyntheticArrayBeamformerCore.contract`` take).  The history before frame 0 is zero velocity.
    ``proc`` is only read, never stepped."""
    from .processors.synthetic_array_beamformer import gate, window_geometry
    vel = np.asarray(velocities, dtype=np.float64)
    if vel.ndim != 2 or vel.shape[1] != 3:
        raise ValueError(f"synthetic_array_geometry: velocities must be [n_frames, 3], got {vel.shape}")
    H, n = int(proc.num_frames), len(vel)
    padded = np.concatenate([np.zeros((H - 1, 3)), vel])
    valid = np.zeros(n, dtype=bool)
    geoms = []
    for f in range(n):
        hist = padded[f:f + H]
        valid[f] = gate(hist, proc.min_vel, proc.max_vel, proc.max_vel_stdev)
        if valid[f]:
            g = window_geometry(hist, proc.chirp_start_times_us, proc.frame_period_ms)
            geoms.append(g.transpose(1, 0, 2).reshape(3, -1))
    E = H * len(proc.chirp_start_times_us)
    return valid, (np.stack(geoms) if geoms else np.zeros((0, 3, E)))


def synthetic_array_patterns(proc, velocities, ctx: _lib.Context = None) -> Tuple[np.ndarray, np.ndarray]:
    """``(frames, patterns)``: the beam pattern float32 ``[n_valid, n_az, n_el]`` that ``proc.compute_synthetic_array_pattern(
    proc.array_geometry)`` gives after each frame whose geometry is valid when a fresh processor like ``proc`` is stepped through
    ``velocities [n, 3]`` -- frames and geometries are those of ``synthetic_array_geometry``, all patterns one
    ``mmw_synth_array_pattern`` call.  No cubes are involved, so ``n`` may be a whole drive.  ``proc`` is only read."""
    valid, P = synthetic_array_geometry(proc, velocities)
    return np.flatnonzero(valid).astype(np.int64), array_patterns(P, proc.d, proc.lambda_m, ctx=ctx)


def _per_frame_pairs(what: str, pairs, n_frames: Optional[int]) -> np.ndarray:
    """``[F][2]`` float64 copy of one pair for all frames or of one pair per frame."""
    arr = np.array(pairs, dtype=np.float64)
    if arr.shape == (2,):
        arr = np.tile(arr, (1 if n_frames is None else n_frames, 1))
    if arr.ndim != 2 or arr.shape[1] != 2 or (n_frames is not None and arr.shape[0] != n_frames):
        want = "[F, 2]" if n_frames is None else f"[{n_frames}, 2] (one pair per resident frame) or one pair"
        raise ValueError(f"doppler_azimuth: {what} must be {want}, got {arr.shape}")
    return arr


def doppler_azimuth_tables(proc, range_windows, precise_vel_ranges=None):
    """Host tables of ``mmw_doppler_azimuth_batch`` / ``mmw_doppler_azimuth_zoom_batch`` for a ``DopplerAzimuthProcessor``.

    ``range_windows [F, 2]`` in metres -> ``rows`` int32 ``[F, 2]``: the interval ``[lo, hi)`` of the range bins ``process`` keeps
    for that window (``keep[0], keep[-1] + 1``; ``lo == hi`` when no bin lies inside).  With ``precise_vel_ranges [F, 2]`` the
    result is ``(rows, freq, m, bins)``: ``freq`` float64 ``[F, M]`` the frequency list of every frame from ``proc._zoom_plan``
    (NaN where the reference emits zeros, and NaN padding behind the ``m[f]`` bins of a frame whose list is shorter than
    ``M = max(m)``), ``bins[f]`` that frame's ``zoomed_vel_bins``.  ``proc`` and the caller's arrays are only read."""
    import copy
    rb = np.asarray(proc.range_bins, dtype=np.float64)
    rw = _per_frame_pairs("range_windows", range_windows, None)
    lo = np.searchsorted(rb, rw[:, 0], side="left")         # first bin >= window start
    hi = np.searchsorted(rb, rw[:, 1], side="right")        # one past the last bin <= window end
    rows = np.stack([lo, np.maximum(hi, lo)], axis=1).astype(np.int32)
    if precise_vel_ranges is None:
        return rows
    pv = _per_frame_pairs("precise_vel_ranges", precise_vel_ranges, None)
    if len(pv) != len(rw):
        raise ValueError(f"doppler_azimuth: {len(rw)} range windows but {len(pv)} velocity ranges")
    plan = copy.copy(proc)              # _zoom_plan sets zoomed_vel_bins: on the copy
    lists, bins = [], []
    for vr in pv:
        lists.append(np.asarray(plan._zoom_plan(vr.copy()), dtype=np.float64))
        bins.append(np.array(plan.zoomed_vel_bins, dtype=np.float64))
    m = np.array([len(x) for x in lists], dtype=np.int64)
    freq = np.full((len(pv), int(m.max()) if len(m) else 0), np.nan)
    for f, x in enumerate(lists):
        freq[f, :len(x)] = x
    return rows, freq, m, bins


def _peak_groups(groups, n_sets: int, shift: np.ndarray) -> np.ndarray:
    """``[G][2]`` int32 table of ``mmw_doppler_azimuth_peaks`` from groups written as a set index, ``(set,)`` or ``(set, set)``."""
    table = []
    for g, grp in enumerate(groups):
        idx = [int(i) for i in np.atleast_1d(np.asarray(grp)).ravel()]
        if len(idx) not in (1, 2):
            raise ValueError(f"doppler_azimuth_peaks: groups[{g}] = {grp!r} must name one set or two")
        if any(not 0 <= i < n_sets for i in idx):
            raise ValueError(f"doppler_azimuth_peaks: groups[{g}] = {grp!r} names a set outside the {n_sets} of rx_sets")
        if len(idx) == 2 and idx[0] == idx[1]:
            raise ValueError(f"doppler_azimuth_peaks: groups[{g}] = {grp!r} names one set twice")
        if len(idx) == 2 and shift[idx[0]] != shift[idx[1]]:
            raise ValueError(f"doppler_azimuth_peaks: groups[{g}] = {grp!r} averages sets that do not share shift_angle")
        table.append(idx + [-1] * (2 - len(idx)))
    return np.array(table, dtype=np.int32).reshape(len(table), 2)


def precise_ranges_from_zero_az(az_zero, el_zero, precise_vel_bound: float = 0.25) -> np.ndarray:
    """The ``[F, 2]`` velocity ranges of the precise pass from the zero-azimuth peaks of a coarse pass: per frame the reference's
    ``estimate_ego_vx_velocity`` (processors/velocity_estimator.py:640-661: minus the mean of the azimuth and the elevation peak
    velocity when both exist, minus the one that exists, else 0) and the ``precise_vel_range`` its ``compute_*_response`` build
    around ``-1 * ego_vx`` (:163-166).  ``az_zero[f]`` / ``el_zero[f]``: what ``detect_peak_zero_az`` returns (``[0.0, vel]`` or an
    empty ``(0, 2)`` array); ``el_zero=None``: no elevation response (a standard array).  Host only."""
    def vels(peaks, n):
        out = np.full(n, np.nan)
        for f, p in enumerate(peaks):
            p = np.asarray(p, dtype=np.float64)
            if p.shape[0] > 0:
                out[f] = p[1]
        return out
    n = len(az_zero)
    if el_zero is not None and len(el_zero) != n:
        raise ValueError(f"precise_ranges_from_zero_az: {n} azimuth peaks but {len(el_zero)} elevation peaks")
    az = vels(az_zero, n)
    el = vels(el_zero, n) if el_zero is not None else np.full(n, np.nan)
    has_az, has_el = ~np.isnan(az), ~np.isnan(el)
    ego = np.zeros(n)
    both = has_az & has_el
    ego[both] = -1 * (az[both] + el[both]) / 2.0
    ego[has_az & ~has_el] = -1 * az[has_az & ~has_el]
    ego[has_el & ~has_az] = -1 * el[has_el & ~has_az]
    centre = -1 * ego
    return np.stack([centre - precise_vel_bound, centre + precise_vel_bound], axis=1)


def _runs(flags: np.ndarray):
    """(start, stop, value) of every run of equal consecutive entries of a bool array."""
    f0 = 0
    for f in range(1, len(flags) + 1):
        if f == len(flags) or flags[f] != flags[f0]:
            yield f0, f, bool(flags[f0])
            f0 = f


class FramePipeline:
    """``[F, V, S, C]`` complex64 cubes in HBM -> RD cube, detections, point clouds, 3-D FFT cube.

    Mirrors ``PointCloudGenerator(RangeDopplerDetector2D(CaCFAR2D/OsCFAR2D))`` and
    ``RangeAngleProcessorDBSEnhanced.compute_3d_windowed_fft`` per frame (reference:
    processors/point_cloud_generator.py:108-140, range_angle_resp_dbs_enhanced.py:137-198).

    ``ground=<RangeDopplerGroundDetector>``: ``detect()`` / ``point_clouds()`` are those of
    ``PointCloudGenerator(detector_type="range_doppler_ground_detector")`` called frame by frame, with the detector's
    Altimeter carried through the batch (and from call to call, and from chunk to chunk of ``stream()``); ``altitudes``
    holds its reported altitude after every frame.  The velocity detector must be a stock 1-D CFAR (CA / OS / GO / SO).

    ``sequential=<RangeDopplerDetectorSequential>``: ``detect()`` / ``point_clouds()`` are those of
    ``PointCloudGenerator(detector_type="range_doppler_detector_sequential")`` called frame by frame.  Only the two CFAR
    parameter sets of the detector are read (both stock 1-D CFARs); its per-frame caches are not touched.

    ``integrate_rx=[v0, v1, ...]`` (no upstream counterpart): the 2-D CFAR of ``cfar=`` runs on the float64
    power summed over the listed virtual antennas, ``sum_v |RD_v|^2`` added in list order, in place of antenna 0's ``|RD|``;
    the angle estimates of the detections are unchanged.  Distinct ints in ``[0, V)``; not with ``ground=`` / ``sequential=``.
    ``integrated_power()`` returns the plane.  ``None`` (the default): the reference's antenna-0 detection.

    ``tdm_compensation=True`` (no upstream counterpart): the cells of every detection are multiplied by the
    conjugate of the phase their transmit slot adds at the detection's Doppler bin before the angle FFT
    (``mmw_angle_argmax_tdm``), in every mode (``cfar=``, ``integrate_rx=``, ``ground=``, ``sequential=``); the detections are
    those of ``detect()``.  ``tdm_tx_slots``: the slot of each virtual antenna (default ``v // num_rx_antennas``).  ``False``
    (the default): the reference's angle estimates, nothing added.

    ``tdm_velocity_unwrap=True`` (with ``tdm_compensation=True``; no upstream counterpart): a target faster than the
    TDM-reduced ``vel_max`` folds back into the plane and would be compensated with the wrong factor.  Each detection is evaluated
    under its ``n_slots`` Doppler hypotheses ``k + h C`` on the deciding list (``tdm_hypothesis_list``: ``"az"``, ``"el"`` or an
    antenna list that spans at least two slots -- it must be a UNIFORM aperture, which is not checked) and the hypothesis with the
    highest angle peak is kept (``mmw_angle_argmax_tdm_hyp``); the other list is compensated with that hypothesis, and the ``v``
    column becomes ``vel_bins[c] + m * 2 vel_max`` (``mmw_tdm_unwrap_velocity``).  ``tdm_hypotheses()`` / ``tdm_unwrapped_bins()``
    return the choices.  ``False`` (the default): nothing added to any path."""

    def __init__(self, config_manager, max_frames: int, shape: Tuple[int, int, int], num_angle_bins: int = 64,
                 cfar=None, az_antenna_idxs=(), el_antenna_idxs=(), shift_az_resp=True, shift_el_resp=False,
                 det_capacity: int = 2048, ctx: _lib.Context = None, ground=None, sequential=None, integrate_rx=None,
                 tdm_compensation: bool = False, tdm_tx_slots=None, tdm_velocity_unwrap: bool = False, tdm_hypothesis_list="az"):
        self.tdm_compensation = bool(tdm_compensation)
        self.tdm_velocity_unwrap = bool(tdm_velocity_unwrap)
        if self.tdm_velocity_unwrap and not self.tdm_compensation:
            raise ValueError("FramePipeline: tdm_velocity_unwrap=True chooses among the factors of tdm_compensation=True; pass both")
        self.tdm_slots = None
        if self.tdm_compensation:
            self.tdm_slots = tdm_tx_slots_of(tdm_tx_slots, int(shape[0]), getattr(config_manager, "num_rx_antennas", 0))
        elif tdm_tx_slots is not None:
            tdm_tx_slots_of(tdm_tx_slots, int(shape[0]), 1)      # (a bad list is refused whether or not it is used)
        self.integrate_rx = None
        if integrate_rx is not None:
            if ground is not None or sequential is not None:
                raise ValueError("FramePipeline: integrate_rx= integrates the plane of the 2-D CFAR (cfar=); it cannot be "
                                 "combined with ground= or sequential=")
            self.integrate_rx = _check_integrate_rx(integrate_rx, int(shape[0]))
        if ground is not None:
            if cfar is not None:
                raise ValueError("FramePipeline: pass either cfar= (2-D detection) or ground= (ground detector), not both")
            _check_ground(ground, tuple(int(x) for x in shape))
        if sequential is not None:
            if cfar is not None or ground is not None:
                raise ValueError("FramePipeline: pass one of cfar= (2-D detection), ground= (ground detector) and "
                                 "sequential= (sequential detector), not several")
            _check_sequential(sequential)
        self.ground = ground
        self.sequential = sequential
        self.altitudes = np.empty(0)
        self.n_flagged = 0      # frames / zoom windows whose peaks the host picked (ground=...)
        self.cm = config_manager
        self.V, self.S, self.C = (int(x) for x in shape)
        self.A = int(num_angle_bins)
        self.max_frames = int(max_frames)
        self.cfar = cfar if cfar is not None else CaCFAR2D((4, 4), (2, 2), 1e-5)
        self.az = [int(i) for i in az_antenna_idxs]
        self.el = [int(i) for i in el_antenna_idxs]
        self.shift_az, self.shift_el = bool(shift_az_resp), bool(shift_el_resp)
        self.tdm_hyp_list = None
        if self.tdm_velocity_unwrap:
            self.tdm_hyp_list = tdm_hypothesis_list_of(tdm_hypothesis_list, self.az, self.el, self.tdm_slots)
        self.cap = int(det_capacity)
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.bufs = _lib.BufferSet(self.ctx)
        self.n_frames = 0
        self.n_refined = 0
        cm = config_manager
        self.vel_bins = np.arange(-cm.vel_max_m_s, cm.vel_max_m_s - cm.vel_res_m_s + 1e-3, cm.vel_res_m_s)
        self.range_bins = np.arange(0, cm.range_max_m - cm.range_res_m / 2 + 1e-3, cm.range_res_m)
        _, self.angle_bins = angle_tables(self.A)
        self.cube_bytes = self.V * self.S * self.C * 8
        self.d_in = self.bufs.get("cubes", self.max_frames * self.cube_bytes)

    # Every way frames become resident (load*, synth, a stream() chunk) ends by setting n_frames: what is remembered about results
    # computed from the cubes before -- the arguments of the last calibration, for synthetic_array_patterns -- is forgotten there.
    @property
    def n_frames(self):
        return self._n_frames

    @n_frames.setter
    def n_frames(self, n):
        self._n_frames = n
        self._synth_calib_key = None

    # ------------------------------------------------------------------ input
    def load(self, cubes: np.ndarray):
        cubes = np.ascontiguousarray(cubes, dtype=np.complex64)
        if cubes.ndim != 4 or cubes.shape[1:] != (self.V, self.S, self.C) or cubes.shape[0] > self.max_frames:
            raise ValueError(f"expected [F<={self.max_frames}, {self.V}, {self.S}, {self.C}] cubes, got {cubes.shape}")
        self.d_in.upload(cubes)
        self.n_frames = cubes.shape[0]

    def load_raw(self, raw_cubes: np.ndarray, num_tx: int):
        """``[F, num_rx, S, num_tx * loops]`` raw cubes (the layout ``VirtualArrayReformatter.process`` consumes,
        virtual_array_reformater.py:44-65): uploaded once, de-interleaved on the device into the virtual-array
        cubes every other method works on.  ``chain3d_raw`` skips even that pass."""
        raw = np.ascontiguousarray(raw_cubes, dtype=np.complex64)
        num_tx = int(num_tx)
        if raw.ndim != 4 or num_tx < 1 or self.V % num_tx or raw.shape[1] != self.V // num_tx or \
                raw.shape[2:] != (self.S, num_tx * self.C) or raw.shape[0] > self.max_frames:
            raise ValueError(f"expected [F<={self.max_frames}, {self.V}/num_tx, {self.S}, num_tx*{self.C}] raw cubes, "
                             f"got {raw.shape} with num_tx={num_tx}")
        self.d_raw = self.bufs.get("raw", self.max_frames * self.cube_bytes)
        self.d_raw.upload(raw)
        self.n_frames, self._raw_tx, self.d_raw_i16 = raw.shape[0], num_tx, None
        _lib.check(self.ctx.lib.mmw_virtual_array_reformat(self.ctx.handle, self.d_raw.ptr, self.d_in.ptr, self.n_frames,
                                                           self.V // num_tx, num_tx, self.S, self.C))

    def load_raw_i16(self, raw_iq: np.ndarray, num_tx: int):
        """``[F, num_rx, S, num_tx * loops, 2]`` int16 I/Q samples: uploaded as they are (half the bytes of complex64)
        and converted + de-interleaved on the device.  No upstream oracle for this layout (the reference receives complex
        cubes from a dataset reader that is not in its tree): it is the raw cube of ``load_raw`` with int16 pairs."""
        raw = np.ascontiguousarray(raw_iq, dtype=np.int16)
        num_tx = int(num_tx)
        if raw.ndim != 5 or raw.shape[4] != 2 or num_tx < 1 or self.V % num_tx or raw.shape[1] != self.V // num_tx or \
                raw.shape[2:4] != (self.S, num_tx * self.C) or raw.shape[0] > self.max_frames:
            raise ValueError(f"expected [F<={self.max_frames}, {self.V}/num_tx, {self.S}, num_tx*{self.C}, 2] int16 samples, "
                             f"got {raw.shape} with num_tx={num_tx}")
        d_i16 = self.bufs.get("raw_i16", self.max_frames * self.cube_bytes // 2)
        d_i16.upload(raw)
        self.n_frames, self._raw_tx, self.d_raw_i16 = raw.shape[0], num_tx, d_i16
        self.d_raw = None
        _lib.check(self.ctx.lib.mmw_virtual_array_reformat_i16(self.ctx.handle, d_i16.ptr, self.d_in.ptr, self.n_frames,
                                                               self.V // num_tx, num_tx, self.S, self.C))

    def stream(self, chunks, work: Callable[["FramePipeline"], object] = None, num_tx: int = 0, pinned: bool = False):
        """Host-resident frame loop (the reference's scripts/test_vel_estimation.py:145-151): iterate ``chunks`` of host cubes
        and yield ``work(self)`` per chunk (default: ``point_clouds()``), with the upload of chunk k + 1 on the copy queue
        while chunk k is processed.

        ``chunks``: ``[F_k <= max_frames, V, S, C]`` complex64 cubes, or -- with ``num_tx > 0`` -- int16 I/Q raw cubes
        ``[F_k, V / num_tx, S, num_tx * C, 2]`` (layout of ``load_raw_i16``: no upstream oracle).  ``pinned=True``: the chunks
        already live in pinned memory (``ctx.host_array``) and are copied from where they are; otherwise each chunk is first
        copied into one of two pinned staging blocks (a host memcpy, usually the slowest stage of the loop)."""
        ctx, Q = self.ctx, _lib
        work = work or (lambda p: p.point_clouds())
        i16 = num_tx > 0
        frame_bytes = self.cube_bytes // 2 if i16 else self.cube_bytes
        dev = [self.bufs.get("stream_in0", self.max_frames * frame_bytes), self.bufs.get("stream_in1", self.max_frames * frame_bytes)]
        ev_up, ev_free = [ctx.event(), ctx.event()], [ctx.event(), ctx.event()]
        # pinned staging blocks live with the pipeline (grow-only, like its device buffers): a per-file loop calling stream()
        # again and again re-uses them instead of pinning max_frames * frame_bytes twice per call
        stage = self.__dict__.setdefault("_stage", [None, None])
        d_cubes_own = self.d_in
        saved_raw = (getattr(self, "d_raw", None), getattr(self, "d_raw_i16", None), getattr(self, "_raw_tx", 0))
        it = iter(chunks)

        def upload(k, chunk):
            b = k % 2
            a = np.asarray(chunk)
            want = np.int16 if i16 else np.complex64
            if a.dtype != want or not a.flags.c_contiguous:
                a = np.ascontiguousarray(a, dtype=want)
            n = a.shape[0]
            if n > self.max_frames or a.nbytes != n * frame_bytes:
                raise ValueError(f"chunk of shape {a.shape} does not hold <= {self.max_frames} frames of {frame_bytes} bytes")
            if k >= 2:
                ctx.wait(Q.QUEUE_COPY, ev_free[b])          # the compute of chunk k - 2 has read device block b
            src = a
            if not pinned:
                if k >= 2:
                    ctx.event_sync(ev_up[b])                 # copy k - 2 has left staging block b
                if stage[b] is None or stage[b].nbytes < self.max_frames * frame_bytes:
                    if stage[b] is not None:
                        ctx.host_free(stage[b])
                    stage[b] = ctx.host_array((self.max_frames * frame_bytes,), np.uint8)
                src = stage[b][:a.nbytes]
                src[:] = a.reshape(-1).view(np.uint8)
            ctx.copy_async(dev[b].ptr, src.ctypes.data, a.nbytes, to_host=False, queue=Q.QUEUE_COPY)
            ctx.record(ev_up[b], Q.QUEUE_COPY)
            return n, src

        nxt = next(it, None)
        k = 0
        pending = upload(0, nxt) if nxt is not None else None
        keep = []                                           # sources of copies in flight stay referenced
        try:
            while pending is not None:
                n, src = pending
                keep = [src]
                nxt = next(it, None)
                pending = upload(k + 1, nxt) if nxt is not None else None
                if pending is not None:
                    keep.append(pending[1])
                b = k % 2
                ctx.wait(Q.QUEUE_COMPUTE, ev_up[b])
                self.n_frames = n
                if i16:
                    self.d_in = d_cubes_own
                    _lib.check(ctx.lib.mmw_virtual_array_reformat_i16(ctx.handle, dev[b].ptr, self.d_in.ptr, n, self.V // num_tx,
                                                                      num_tx, self.S, self.C))
                    # work() may call chain3d_raw(): it reads THIS chunk's raw samples
                    self.d_raw, self.d_raw_i16, self._raw_tx = None, dev[b], num_tx
                else:
                    self.d_in = dev[b]
                    self.d_raw = self.d_raw_i16 = None     # no raw cube behind a streamed virtual-array chunk
                out = work(self)
                ctx.record(ev_free[b], Q.QUEUE_COMPUTE)
                yield out
                k += 1
        finally:
            self.d_in = d_cubes_own
            self.d_raw, self.d_raw_i16, self._raw_tx = saved_raw
            ctx.sync()
            for e in ev_up + ev_free:
                _lib.check(ctx.lib.mmw_event_destroy(ctx.handle, e))

    def chain3d_raw(self, magnitude: bool = False):
        """3-D windowed FFT straight from the raw cubes of ``load_raw`` / ``load_raw_i16`` (``mmw_chain3d_raw[_i16]``)."""
        F, A, S, C = self.n_frames, self.A, self.S, self.C
        self.d_cube3d = self.bufs.get("cube3d", max(F, 1) * A * S * C * (4 if magnitude else 8))
        self._cube3d_mag = magnitude
        if getattr(self, "d_raw_i16", None) is None and getattr(self, "d_raw", None) is None:
            raise ValueError("chain3d_raw() needs the raw cubes of load_raw() / load_raw_i16() (or an int16 stream() chunk)")
        if getattr(self, "d_raw_i16", None) is not None:        # int16 cells: converted inside the first kernel's loads
            _lib.check(self.ctx.lib.mmw_chain3d_raw_i16(self.ctx.handle, self.d_raw_i16.ptr, None, self.d_cube3d.ptr, F,
                                                        self.V // self._raw_tx, self._raw_tx, S, C, A, int(magnitude)))
            return
        _lib.check(self.ctx.lib.mmw_chain3d_raw(self.ctx.handle, self.d_raw.ptr, None, self.d_cube3d.ptr, F,
                                                self.V // self._raw_tx, self._raw_tx, S, C, A, int(magnitude)))

    def synth(self, n_frames: int, seed0: int, num_targets: int = 8, noise_sigma: float = 30.0):
        if n_frames > self.max_frames:
            raise ValueError("n_frames exceeds max_frames")
        _lib.check(self.ctx.lib.mmw_synth_cubes(self.ctx.handle, self.d_in.ptr, n_frames, self.V, self.S, self.C,
                                                int(seed0), int(num_targets), float(noise_sigma)))
        self.n_frames = n_frames

    def cubes(self, lo: int = 0, hi: Optional[int] = None) -> np.ndarray:
        hi = self.n_frames if hi is None else hi
        return self.d_in.download((hi - lo, self.V, self.S, self.C), np.complex64, lo * self.cube_bytes)

    # ------------------------------------------------------------------ compute
    def chain3d(self, magnitude: bool = False):
        """3-D windowed FFT of every frame; result stays on the device (``fetch_chain3d`` copies frames out)."""
        F, A, S, C = self.n_frames, self.A, self.S, self.C
        esz = 4 if magnitude else 8
        self.d_cube3d = self.bufs.get("cube3d", max(F, 1) * A * S * C * esz)
        self._cube3d_mag = magnitude
        _lib.check(self.ctx.lib.mmw_chain3d(self.ctx.handle, self.d_in.ptr, None, self.d_cube3d.ptr, F, self.V, S, C, A,
                                            int(magnitude)))

    def fetch_chain3d(self, frame: int) -> np.ndarray:
        A, S, C = self.A, self.S, self.C
        if self._cube3d_mag:
            return self.d_cube3d.download((A, S, C), np.float32, frame * A * S * C * 4)
        return self.d_cube3d.download((A, S, C), np.complex64, frame * A * S * C * 8)

    def _dbs_launch(self, dbs, velocities_ned, rx_antennas, chirp_idx, with_slow: bool = True):
        """Argument checks, host tables and launches of ``dbs_range_angle`` / ``dbs_range_angle_device``; no download.
        ``with_slow=False`` leaves the plain range-angle response of the slow frames out."""
        from .processors.range_angle_resp_dbs_enhanced import RangeAngleProcessorDBSEnhanced
        # every argument check comes before the first use of self.ctx / self.bufs (tests/test_dbs_batch_host.py calls this
        # on a pipeline that has no device behind it)
        if not isinstance(dbs, RangeAngleProcessorDBSEnhanced):
            raise ValueError(f"dbs_range_angle: dbs must be a RangeAngleProcessorDBSEnhanced, got {type(dbs).__name__}")
        F, V, S, C = self.n_frames, self.V, self.S, self.C
        v = np.asarray(velocities_ned, dtype=np.float64)
        if v.ndim != 2 or v.shape != (F, 3):
            raise ValueError(f"dbs_range_angle: velocities_ned must be [{F}, 3] (one NED velocity per resident frame), got {v.shape}")
        rx = np.asarray(rx_antennas).astype(int).ravel()
        if np.any((rx < -V) | (rx >= V)):
            raise ValueError(f"dbs_range_angle: rx_antennas {rx.tolist()} hold an index outside the {V} antennas")
        A = int(dbs.num_angle_bins)
        n = rx.size if rx.size else V
        if A < n:
            raise ValueError(f"dbs_range_angle: dbs.num_angle_bins ({A}) must be >= number of antennas ({n})")
        n_out = int(len(dbs.angle_bins_dbs_enhanced))
        sharp = dbs_branches(dbs, v)
        ang_tab, vel_tab = dbs_index_tables(dbs, v[sharp])
        self.dbs_sharpened = sharp
        self._dbs_shape = (A, n_out)
        self.d_dbs = self.bufs.get("dbs_out", max(F, 1) * S * max(n_out, 1) * 4)
        with_slow = with_slow and not np.all(sharp)
        d_ra = self.bufs.get("dbs_ra", int(np.count_nonzero(~sharp)) * S * A * 4) if with_slow else None
        rx_pos, n_rx = _lib.int_array(rx % V)
        rx_raw, _ = _lib.int_array(rx)
        lib, h = self.ctx.lib, self.ctx.handle
        done, slow_at = 0, {}
        for f0, f1, fast in _runs(sharp):
            cubes = self.d_in.at(f0 * self.cube_bytes)
            if fast:
                a_rows, v_rows = ang_tab[done:done + f1 - f0], vel_tab[done:done + f1 - f0]
                done += f1 - f0
                _lib.check(lib.mmw_dbs_sharpen(h, cubes, None, a_rows.ctypes.data_as(_lib._ip), v_rows.ctypes.data_as(_lib._ip),
                                               self.d_dbs.at(f0 * S * n_out * 4), f1 - f0, V, S, C, A, rx_pos, n_rx, n_out))
            elif with_slow:
                slot = len(slow_at)
                _lib.check(lib.mmw_range_angle(h, cubes, d_ra.at(slot * S * A * 4), f1 - f0, V, S, C, A, int(chirp_idx),
                                               rx_raw, n_rx, 1))
                slow_at.update({f: slot + f - f0 for f in range(f0, f1)})
        return d_ra, slow_at

    def dbs_range_angle(self, dbs, velocities_ned, rx_antennas=(), chirp_idx: int = 0) -> List[np.ndarray]:
        """``dbs.process(cube_f, velocity_ned=velocities_ned[f], rx_antennas=..., chirp_idx=...)`` of every resident frame
        (reference: range_angle_resp_dbs_enhanced.py:308-342, driven per frame by scripts/doppler_deam_sharpening_demo.py).

        ``dbs``: a ``RangeAngleProcessorDBSEnhanced``; only its bin tables, ``num_angle_bins`` and ``min_vel_dbs`` are read.
        ``velocities_ned``: ``[n_frames, 3]``, used as given (``ego_velocities()`` reports the sensor frame: the caller converts,
        as the caller of the reference does).  Returns ``n_frames`` float64 arrays: ``[S, n_out]`` sharpened
        (``mmw_dbs_sharpen``: a single-bin angle DFT per pixel on the batch's range-Doppler cubes, no ``[A, S, C]`` cube) where
        the horizontal speed is not below ``dbs.min_vel_dbs``, else the plain ``[S, A]`` range-angle response of chirp
        ``chirp_idx`` (``mmw_range_angle``, one call per run of consecutive slow frames).  ``self.dbs_sharpened`` (bool
        ``[n_frames]``) says which.  The index tables of all frames are made at once by ``dbs_index_tables`` and equal
        ``dbs._dbs_indices`` per frame.  The resident cubes are not changed."""
        d_ra, slow_at = self._dbs_launch(dbs, velocities_ned, rx_antennas, chirp_idx)
        F, S = self.n_frames, self.S
        A, n_out = self._dbs_shape
        out: List[np.ndarray] = [None] * F
        for f0, f1, fast in _runs(self.dbs_sharpened):
            if fast:
                block = self.d_dbs.download((f1 - f0, S, n_out), np.float32, f0 * S * n_out * 4).astype(np.float64)
            else:
                block = d_ra.download((f1 - f0, S, A), np.float32, slow_at[f0] * S * A * 4).astype(np.float64)
            for f in range(f0, f1):
                out[f] = block[f - f0]
        return out

    def dbs_range_angle_device(self, dbs, velocities_ned, rx_antennas=(), chirp_idx: int = 0) -> _lib.DeviceBuffer:
        """The sharpened images of ``dbs_range_angle`` left in HBM: float32 ``[n_frames][S][n_out]``, no download.  The rows of
        frames below ``dbs.min_vel_dbs`` are NOT written (``self.dbs_sharpened`` says which frames they are)."""
        self._dbs_launch(dbs, velocities_ned, rx_antennas, chirp_idx, with_slow=False)
        return self.d_dbs

    def micro_doppler_device(self, target_ranges=(0, 1.0), rx_idx: int = 0) -> _lib.DeviceBuffer:
        """The micro-Doppler rows of ``micro_doppler`` left in HBM: float32 ``[n_frames][C]``, nothing downloaded."""
        from .processors.micro_doppler_resp import window_rows
        # every argument check comes before the first use of self.ctx / self.bufs
        _, lo, hi = window_rows(self.range_bins, target_ranges)
        if len(self.range_bins) != self.S or len(self.vel_bins) != self.C:
            raise ValueError(f"micro_doppler: cubes of {self.S} samples x {self.C} chirps do not match the configuration's "
                             f"{len(self.range_bins)} range bins x {len(self.vel_bins)} velocity bins")
        rx = int(rx_idx)
        if not -self.V <= rx < self.V:
            raise IndexError(f"micro_doppler: rx_idx {rx_idx} is out of bounds for {self.V} antennas")
        self.d_micro = self.bufs.get("micro_doppler", max(self.n_frames, 1) * self.C * 4)
        _lib.check(self.ctx.lib.mmw_micro_doppler(self.ctx.handle, self.d_in.ptr, self.d_micro.ptr, self.n_frames, self.V, self.S,
                                                  self.C, rx % self.V, lo, hi))
        return self.d_micro

    def micro_doppler(self, target_ranges=(0, 1.0), rx_idx: int = 0) -> np.ndarray:
        """Row f of the float64 ``[n_frames, C]`` result is what ``MicroDopplerProcessor(cm, target_ranges).process(cube_f, rx_idx)``
        puts into column 0 of its spectrogram (reference: processors/micro_doppler_resp.py:91-114, stepped per frame by every
        movie and viewer loop): ``max`` over the range rows of the window of ``|fftshift_C(fft2(cube_f[rx_idx]))|``, from one
        ``mmw_micro_doppler`` call on the resident cubes.  The rows do not depend on each other: ``micro_doppler_history(rows,
        H)`` is the processor's buffer after these frames.  Works on whatever ``load`` / ``load_raw`` / ``load_raw_i16`` /
        ``synth`` / a ``stream()`` chunk left resident; ``cfar=``, ``ground=`` and ``sequential=`` play no part."""
        d = self.micro_doppler_device(target_ranges, rx_idx)
        return d.download((self.n_frames, self.C), np.float32).astype(np.float64)

    def strip_map_sar_device(self, proc, velocities, sensor_height_m: float = 0.24, rx_index: int = 0,
                             max_SAR_distance: float = 1.5):
        """The SAR slices of ``strip_map_sar`` left in HBM, nothing downloaded: ``(d_out, h_off, windows)`` -- the packed complex64
        buffer, the int64 ``[n_frames + 1]`` element offsets of the frames' blocks in it and the int32 ``[n_frames, 4]`` windows
        (row_lo, row_hi, col_lo, col_hi; half open).  Block f is row-major ``[row_hi - row_lo][col_hi - col_lo]``."""
        from .processors.strip_map_SAR_processor import StripMapSARProcessor, frame_windows, sar_slices_call
        # every argument check comes before the first use of self.ctx / self.bufs
        if not isinstance(proc, StripMapSARProcessor):
            raise ValueError(f"strip_map_sar: proc must be a StripMapSARProcessor, got {type(proc).__name__}")
        F = self.n_frames
        vel = np.asarray(velocities, dtype=np.float64)
        if vel.ndim == 0:
            vel = np.full(F, float(vel))
        if vel.shape != (F,):
            raise ValueError(f"strip_map_sar: velocities must be {F} numbers (one per resident frame) or one, got shape {vel.shape}")
        rx = int(rx_index)
        if not -self.V <= rx < self.V:
            raise IndexError(f"strip_map_sar: rx_index {rx_index} is out of bounds for {self.V} antennas")
        win, off = frame_windows(proc, vel, sensor_height_m, max_SAR_distance, self.S, self.C)
        self.d_sar = self.bufs.get("sar_slices", max(int(off[-1]), 1) * 8)
        sar_slices_call(self.ctx, self.d_in.ptr, F, self.V, self.S, self.C, rx % self.V, win, off, self.d_sar.ptr)
        return self.d_sar, off, win

    def strip_map_sar(self, proc, velocities, sensor_height_m: float = 0.24, rx_index: int = 0, max_SAR_distance: float = 1.5):
        """``(slices, windows)``: entry f of the list ``slices`` is ``proc.process(cube_f, velocities[f], sensor_height_m, rx_index,
        max_SAR_distance)`` of ``StripMapSARProcessor`` (reference: processors/strip_map_SAR_processor.py:160-194) -- complex128, the
        shape of that frame's window, which moves with the frame's platform speed -- from one ``mmw_sar_slices`` call on the
        resident (virtual-array) cubes and one download.  ``velocities`` is ``[n_frames]`` or one number for all frames;
        ``windows`` is the int32 ``[n_frames, 4]`` table of ``strip_map_sar_device``.  Only ``proc``'s tables are read: its
        ``valid_*_slice`` / mesh attributes stay what its last own call left (``proc.geometry(v)`` gives any frame's).  An
        ``IndexError`` of the geometry (no range bin between height and distance) comes out as it does per frame."""
        d, off, win = self.strip_map_sar_device(proc, velocities, sensor_height_m, rx_index, max_SAR_distance)
        flat = d.download((int(off[-1]),), np.complex64).astype(np.complex128) if off[-1] else np.zeros(0, dtype=np.complex128)
        return [flat[off[f]:off[f + 1]].reshape(win[f, 1] - win[f, 0], win[f, 3] - win[f, 2]) for f in range(len(win))], win

    def range_detections(self, detector, chirp_idx: int = 0, return_thresholds: bool = False):
        """Entry f of the returned list is ``RangeDetector.process(cube_f)`` of ``detector`` (reference:
        processors/range_detector.py:59-83): the ascending int array of the range cells above their 1-D CFAR threshold on the
        float64 range profile of chirp ``chirp_idx`` (the class uses chirp 0), from one ``mmw_range_detect`` call.
        ``return_thresholds=True``: ``(dets, thresholds)`` with the float64 ``[n_frames, S]`` thresholds; ``self.range_profiles``
        holds the float64 ``[n_frames, S]`` profiles either way.  Only the parameters of ``detector.cfar_detector`` are read.  A
        detector the device cannot stand in for (a subclass, its own ``_compute_thresholds``) runs its own ``detect`` on each
        downloaded profile instead."""
        from .processors.range_detector import RangeDetector, device_cfar1d_args
        # every argument check comes before the first use of self.ctx / self.bufs
        if not isinstance(detector, RangeDetector):
            raise ValueError(f"range_detections: detector must be a RangeDetector, got {type(detector).__name__}")
        chirp = int(chirp_idx)
        if not -self.C <= chirp < self.C:
            raise IndexError(f"range_detections: chirp_idx {chirp_idx} is out of bounds for {self.C} chirps")
        F, V, S, C = self.n_frames, self.V, self.S, self.C
        args = device_cfar1d_args(detector.cfar_detector)
        lib, h = self.ctx.lib, self.ctx.handle
        d_prof = self.bufs.get("range_profile64", max(F, 1) * S * 8)
        if args is None:
            _lib.check(lib.mmw_range_profile_f64(h, self.d_in.ptr, d_prof.ptr, F, V, S, C, chirp))
            self.range_profiles = d_prof.download((F, S), np.float64)
            dets, thr = [], np.zeros((F, S))
            for f in range(F):
                dets.append(np.asarray(detector.cfar_detector.detect(self.range_profiles[f]), dtype=int))
                thr[f] = detector.cfar_detector.thresholds
            return (dets, thr) if return_thresholds else dets
        kind, T, G, scale, k = args
        d_thr = self.bufs.get("range_thr64", max(F, 1) * S * 8) if return_thresholds else None
        d_dets, d_cnt = self.bufs.get("range_dets", max(F, 1) * S * 4), self.bufs.get("range_counts", max(F, 1) * 4)
        _lib.check(lib.mmw_range_detect(h, self.d_in.ptr, F, V, S, C, chirp, kind, T, G, scale, k, d_prof.ptr,
                                        d_thr.ptr if d_thr is not None else None, d_dets.ptr, d_cnt.ptr, S))
        self.range_profiles = d_prof.download((F, S), np.float64)
        counts = d_cnt.download((F,), np.int32)
        table = d_dets.download((F, S), np.int32)
        dets = [table[f, :counts[f]].astype(int) for f in range(F)]
        return (dets, d_thr.download((F, S), np.float64)) if return_thresholds else dets

    def capon_range_angle_device(self, thetas_rad, rx_antennas, range_bins=None, delta: float = 1e-3,
                                 perform_windowing: bool = True, frames_per_pass: Optional[int] = None) -> _lib.DeviceBuffer:
        """The Capon maps of ``capon_range_angle`` left in HBM: float32 ``[n_frames][R_w][T]``, nothing downloaded."""
        # every argument check comes before the first use of self.ctx / self.bufs
        th, rx, (r_lo, r_hi), delta, fpp = capon_cube_args(self.V, self.S, thetas_rad, rx_antennas, range_bins, delta,
                                                           frames_per_pass)
        F, Rw, T = self.n_frames, r_hi - r_lo, len(th)
        if fpp is None:
            fpp = capon_pass_frames(len(rx), Rw, self.C)
        fpp = max(1, min(fpp, F))
        self._capon_shape = (F, Rw, T)
        self.d_capon = self.bufs.get("capon_ra", max(F, 1) * Rw * T * 4)
        d_snap = self.bufs.get("capon_snap", fpp * len(rx) * Rw * self.C * 8)
        capon_from_cubes(self.ctx, self.d_in.ptr, d_snap, self.d_capon, F, (self.V, self.S, self.C), th, rx, (r_lo, r_hi), delta,
                         perform_windowing, fpp)
        return self.d_capon

    def capon_range_angle(self, thetas_rad, rx_antennas, range_bins=None, delta: float = 1e-3, perform_windowing: bool = True,
                          frames_per_pass: Optional[int] = None) -> np.ndarray:
        """Capon / MVDR range-azimuth map of every resident frame, float64 ``[n_frames, R_w, T]``: row ``r - r_lo`` of frame f
        is ``CaponBeamformer(thetas_rad, delta).process(X_f)[r - r_lo]`` on the snapshots ``X_f[i][r - r_lo][k]`` = bin r of the
        (Hann-windowed, unless ``perform_windowing=False``) range FFT of chirp k of antenna ``rx_antennas[i]`` -- with the
        snapshots made on the device from the resident cubes instead of on the host (no upstream implementation exists; the
        definition is DESIGN.md 4.20).  ``rx_antennas``: the ordered azimuth row of the virtual array, 1..16 indices, a
        half-wavelength uniform line array in list order.  ``range_bins=(r_lo, r_hi)``: bin indices, default the whole profile.

        Two calls per pass of ``frames_per_pass`` frames (default ``capon_pass_frames``: a 1 GiB snapshot budget, the fastest
        of the pass sizes measured in DESIGN.md 4.20), on the context's queue in order:
        ``mmw_range_snapshots`` into one scratch buffer, ``mmw_capon`` from it into the pass's slice of the result.  A frame's
        map does not depend on the pass it is in.  Works on whatever ``load`` / ``load_raw`` / ``load_raw_i16`` / ``synth`` / a
        ``stream()`` chunk left resident; ``cfar=``, ``ground=`` and ``sequential=`` play no part."""
        d = self.capon_range_angle_device(thetas_rad, rx_antennas, range_bins, delta, perform_windowing, frames_per_pass)
        if self.n_frames == 0:
            return np.zeros(self._capon_shape)
        return d.download(self._capon_shape, np.float32).astype(np.float64)

    def capon_point_clouds_device(self, thetas_rad, rx_antennas, detector, range_bins=None, delta: float = 1e-3,
                                  perform_windowing: bool = True, doppler_windowing: bool = True,
                                  frames_per_pass: Optional[int] = None) -> _lib.DeviceBuffer:
        """The point clouds of ``capon_point_clouds`` left in HBM: a packed float64 ``[n_frames][det_capacity][4]`` buffer of
        (x, y, z, velocity) rows, frame f holding its ``capon_counts[f]`` points first and zeros behind them.  The detections
        (``d_capon_dets`` int32 ``[F][cap][2]`` (row of the window, angle index), ``d_capon_cnt``), their Doppler bins
        (``d_capon_dop``) and peaks (``d_capon_peak``) and the float32 maps (``d_capon``) stay on the device too; the counts are
        downloaded (``capon_counts``) and a frame with more detections than ``det_capacity`` raises as ``detect()`` does."""
        # every argument check comes before the first use of self.ctx / self.bufs
        th, rx, (r_lo, r_hi), delta, fpp, cfar, cap = capon_points_args(self.V, self.S, self.C, thetas_rad, rx_antennas, detector,
                                                                        range_bins, delta, frames_per_pass, self.cap)
        if len(self.range_bins) < r_hi or len(self.vel_bins) != self.C:
            raise ValueError(f"capon_point_clouds: the config's {len(self.range_bins)} range bins / {len(self.vel_bins)} velocity bins "
                             f"do not serve range bin {r_hi - 1} / {self.C} chirps (config and cube shape disagree)")
        F, Rw, T, n, K = self.n_frames, r_hi - r_lo, len(th), len(rx), self.C
        if fpp is None:
            fpp = capon_pass_frames(n, Rw, K)
        fpp = max(1, min(fpp, F, CAPON_POINTS_PASS_FRAMES))
        lib, h, bufs, F1 = self.ctx.lib, self.ctx.handle, self.bufs, max(F, 1)
        self._capon_shape = (F, Rw, T)
        self.d_capon = bufs.get("capon_ra", F1 * Rw * T * 4)
        d_snap = bufs.get("capon_snap", fpp * n * Rw * K * 8)
        d_map64, d_mask = bufs.get("capon_map64", fpp * Rw * T * 8), bufs.get("capon_mask", fpp * Rw * T)
        self.d_capon_dets, self.d_capon_cnt = bufs.get("capon_dets", F1 * cap * 8), bufs.get("capon_counts", F1 * 4)
        self.d_capon_dop, self.d_capon_peak = bufs.get("capon_dop", F1 * cap * 4), bufs.get("capon_peak", F1 * cap * 8)
        self.d_capon_points = bufs.get("capon_points", F1 * cap * 32)
        rows = np.ascontiguousarray(self.range_bins[r_lo:r_hi], dtype=np.float64)
        vel = np.ascontiguousarray(self.vel_bins, dtype=np.float64)
        d_rng, d_vel = bufs.get("capon_range_tab", rows.nbytes), bufs.get("capon_vel_tab", vel.nbytes)
        d_rng.upload(rows)          # float64 tables made on the host (no device libm)
        d_vel.upload(vel)
        kind, tr, ta, gr, ga, scale, k_rank = cfar
        rx_arr, _ = _lib.int_array(rx)
        th_ptr = th.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        for f0, f1 in capon_passes(F, fpp):
            nf = f1 - f0
            d_map = self.d_capon.at(f0 * Rw * T * 4)
            _lib.check(lib.mmw_range_snapshots(h, self.d_in.at(f0 * self.cube_bytes), d_snap.ptr, nf, self.V, self.S, K, rx_arr, n,
                                               r_lo, r_hi, int(bool(perform_windowing))))
            _lib.check(lib.mmw_capon(h, d_snap.ptr, th_ptr, d_map, nf, n, Rw, K, T, delta))
            _lib.check(lib.mmw_widen_f32_f64(h, d_map, d_map64.ptr, nf * Rw * T))
            _lib.check(lib.mmw_cfar2d(h, d_map64.ptr, None, None, d_mask.ptr, nf, Rw, T, kind, tr, ta, gr, ga, scale, k_rank))
            _lib.check(lib.mmw_compact2d(h, d_mask.ptr, self.d_capon_dets.at(f0 * cap * 8), self.d_capon_cnt.at(f0 * 4), nf, Rw, T, cap))
            capon_doppler_on(self.ctx, d_snap.ptr, self.d_capon_dets.at(f0 * cap * 8), self.d_capon_cnt.at(f0 * 4), th,
                             self.d_capon_dop.at(f0 * cap * 4), self.d_capon_peak.at(f0 * cap * 8), None,
                             self.d_capon_points.at(f0 * cap * 32), d_rng.ptr, d_vel.ptr, nf, n, Rw, K, cap, delta, doppler_windowing)
        self._capon_window = (r_lo, r_hi)
        self.capon_counts = self.d_capon_cnt.download((F,), np.int32) if F else np.zeros(0, np.int32)
        if np.any(self.capon_counts > cap):
            raise _lib.MmwGpuError(f"detection capacity {cap} exceeded (max count {int(self.capon_counts.max())}): "
                                   "raise det_capacity")
        return self.d_capon_points

    def capon_point_clouds(self, thetas_rad, rx_antennas, detector, range_bins=None, delta: float = 1e-3,
                           perform_windowing: bool = True, doppler_windowing: bool = True,
                           frames_per_pass: Optional[int] = None) -> List[np.ndarray]:
        """Point clouds from the Capon / MVDR range-azimuth map of every resident frame: per-frame float64 ``(N, 4)`` arrays of
        (x, y, z, velocity) rows (no upstream implementation exists; the definition is DESIGN.md 4.28).  Per frame: the map of
        ``capon_range_angle`` as float64, ``detector`` (a stock ``CaCFAR2D`` / ``OsCFAR2D`` whose ``num_train`` / ``num_guard``
        are (range, angle) pairs) on it, and for every detection (range bin r, angle index t), in ``detector.detect``'s
        row-major order, the Doppler spectrum of the chirp sequence beamformed with the MVDR weights of that cell
        (``CaponBeamformer.beamformed_doppler``; Hann over the chirps unless ``doppler_windowing=False``).  The point is
        ``(rng cos(theta_t), rng sin(theta_t), 0, vel_bins[dop])`` with ``rng = range_bins[r]``: theta enters with the sign it
        has in ``thetas_rad``, which puts a target on the side ``PointCloudGenerator``'s azimuth puts it for the same cube.  A
        range row whose covariance is not positive definite (an all-zero row, a NaN) gives velocity NaN.

        Sets ``capon_dets`` (per-frame int64 ``(N, 2)``: absolute range bin, angle index), ``capon_doppler_idx`` (int64 ``(N,)``,
        -1 where the row is degenerate) and ``capon_peak`` (float64 ``(N,)``).  The returned lists are valid input to
        ``ego_velocities(estimator, point_clouds=...)`` and ``vehicle_velocities(estimator, point_clouds=...)``.

        Per pass of ``frames_per_pass`` frames (default ``capon_pass_frames``), on the context's queue in order and without a host
        round trip: ``mmw_range_snapshots``, ``mmw_capon``, ``mmw_widen_f32_f64``, ``mmw_cfar2d`` (mask only),
        ``mmw_compact2d``, ``mmw_capon_doppler``.  A frame's result does not depend on the pass it is in.  A frame with more
        detections than ``det_capacity`` raises ``MmwGpuError`` as ``detect()`` does."""
        d = self.capon_point_clouds_device(thetas_rad, rx_antennas, detector, range_bins, delta, perform_windowing,
                                           doppler_windowing, frames_per_pass)
        F, cap, counts, r_lo = self.n_frames, self.cap, self.capon_counts, self._capon_window[0]
        if F == 0:
            self.capon_dets, self.capon_doppler_idx, self.capon_peak = [], [], []
            return []
        pts = d.download((F, cap, 4), np.float64)
        dets = self.d_capon_dets.download((F, cap, 2), np.int32)
        dop = self.d_capon_dop.download((F, cap), np.int32)
        peak = self.d_capon_peak.download((F, cap), np.float64)
        self.capon_dets = [dets[f, :n].astype(np.int64) + np.array([r_lo, 0]) for f, n in enumerate(counts)]
        self.capon_doppler_idx = [dop[f, :n].astype(np.int64) for f, n in enumerate(counts)]
        self.capon_peak = [peak[f, :n].copy() for f, n in enumerate(counts)]
        return [pts[f, :n].copy() if n else np.empty((0, 4)) for f, n in enumerate(counts)]

    def doppler_azimuth_device(self, proc, rx_sets, range_windows, shift_angle=True, precise_vel_ranges=None):
        """The maps of ``doppler_azimuth`` left in HBM, nothing downloaded: ``(buffer, (n_sets, F, rows, 64), m, bins)`` with the
        buffer float32 ``[n_sets][F][rows][64]`` before the valid-angle mask, ``rows = C`` (coarse; ``m`` and ``bins`` are None) or
        the longest frequency list of the batch (precise; frame f holds ``m[f]`` bins, zeros behind them)."""
        from .processors.doppler_azimuth_resp import DopplerAzimuthProcessor
        # every argument check comes before the first use of self.ctx / self.bufs
        if not isinstance(proc, DopplerAzimuthProcessor):
            raise ValueError(f"doppler_azimuth: proc must be a DopplerAzimuthProcessor, got {type(proc).__name__}")
        F, V, S, C = self.n_frames, self.V, self.S, self.C
        A = int(proc.num_angle_bins)
        if A != 64:
            raise ValueError(f"doppler_azimuth: the batch form is built for num_angle_bins == 64, the processor has {A}")
        if len(proc.range_bins) != S:
            raise ValueError(f"doppler_azimuth: cubes of {S} samples do not match the configuration's {len(proc.range_bins)} range bins")
        sets = [np.asarray(s).astype(int).ravel() for s in rx_sets]
        if any(len(s) != len(sets[0]) or len(s) == 0 for s in sets):
            raise ValueError(f"doppler_azimuth: rx_sets must be antenna lists of one length, got lengths {[len(s) for s in sets]}")
        n_sets, n_rx = max(len(sets), 1), (len(sets[0]) if sets else 0)
        if (n_rx if sets else V) > 16:
            raise ValueError(f"doppler_azimuth: a set holds {n_rx if sets else V} antennas: at most 16")
        for k, s in enumerate(sets):
            if np.any((s < -V) | (s >= V)):
                raise ValueError(f"doppler_azimuth: rx_sets[{k}] = {s.tolist()} holds an index outside the {V} antennas")
            if len(np.unique(s % V)) != len(s):
                raise ValueError(f"doppler_azimuth: rx_sets[{k}] = {s.tolist()} repeats an antenna")
        shift = np.atleast_1d(np.asarray(shift_angle, dtype=bool))
        if shift.shape == (1,):
            shift = np.repeat(shift, n_sets)
        if shift.shape != (n_sets,):
            raise ValueError(f"doppler_azimuth: shift_angle must be a bool or one per set ({n_sets}), got {shift.shape}")
        rw = _per_frame_pairs("range_windows", range_windows, F)
        precise = precise_vel_ranges is not None
        m = bins = None
        if precise:
            pv = _per_frame_pairs("precise_vel_ranges", precise_vel_ranges, F)
            n_used = int(proc.vel_bins.size)
            if n_used > C:
                raise ValueError(f"CZT defined for length {n_used}, not {C}")
            rows, freq, m, bins = doppler_azimuth_tables(proc, rw, pv)
            n_rows = int(freq.shape[1])
        else:
            rows = doppler_azimuth_tables(proc, rw)
            n_rows = C
        cm = proc.config_manager
        flags = 0 if (cm.array_geometry == "standard" and cm.virtual_antennas_enabled) else _lib.ANGLE_NO_WINDOW
        rx = np.ascontiguousarray(np.stack(sets) % V if sets else np.zeros((1, 1)), dtype=np.int32)
        set_flags = np.ascontiguousarray(np.where(shift, 0, _lib.ANGLE_NO_SHIFT), dtype=np.int32)
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        shape = (n_sets, F, n_rows, A)
        if F == 0 or n_rows == 0:
            return None, shape, m, bins
        self.d_dopaz = self.bufs.get("dopaz_batch", n_sets * F * n_rows * A * 4)
        ip = lambda a: a.ctypes.data_as(_lib._ip)      # noqa: E731
        lib, h = self.ctx.lib, self.ctx.handle
        if precise:
            freq = np.ascontiguousarray(freq, dtype=np.float64)
            _lib.check(lib.mmw_doppler_azimuth_zoom_batch(h, self.d_in.ptr, self.d_dopaz.ptr, F, V, S, C, A, ip(rx), n_sets, n_rx,
                                                          ip(set_flags), ip(rows), flags, n_used,
                                                          freq.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n_rows))
        else:
            _lib.check(lib.mmw_doppler_azimuth_batch(h, self.d_in.ptr, self.d_dopaz.ptr, F, V, S, C, A, ip(rx), n_sets, n_rx,
                                                     ip(set_flags), ip(rows), flags))
        return self.d_dopaz, shape, m, bins

    def doppler_azimuth(self, proc, rx_sets, range_windows, shift_angle=True, precise_vel_ranges=None):
        """``proc.process(cube_f, rx_antennas=rx_sets[k], range_window=range_windows[f], shift_angle=shift_angle[k], ...)`` of every
        resident frame f and antenna set k (reference: processors/doppler_azimuth_resp.py:419-491, stepped up to eight times per
        frame by the Doppler-azimuth ego-velocity loop, processors/velocity_estimator.py:800-845), from ONE range(-Doppler) pass
        over the resident cubes for all sets.

        ``rx_sets``: equal-length antenna lists, or ``()`` for all antennas; ``range_windows``: ``[F, 2]`` metres or one pair;
        ``shift_angle``: a bool or one per set.  Coarse mode returns float64 ``[n_sets, F, C, n_valid_angles]``; a frame whose
        window holds no range bin is NaN.  With ``precise_vel_ranges`` (``[F, 2]`` or one pair: ``use_precise_fft=True``) the
        result is ``(maps, zoomed_bins)``: ``zoomed_bins[f]`` are that frame's ``zoomed_vel_bins`` and its map is cut to their
        count -- one ``[n_sets, F, m, n_valid]`` array when all frames have ``m`` bins, else a list of ``[n_sets, m_f, n_valid]``
        arrays.  ``proc`` is only read (``proc.zoomed_vel_bins`` stays as it was).  Works on whatever ``load*`` / ``synth`` / a
        ``stream()`` chunk left resident.  ``doppler_azimuth_peaks`` picks the peaks of these maps on the device; the regression of
        the reference's estimator stays on the host."""
        d, shape, m, bins = self.doppler_azimuth_device(proc, rx_sets, range_windows, shift_angle, precise_vel_ranges)
        mask = np.asarray(proc.valid_angle_mask, dtype=bool)
        full = d.download(shape, np.float32).astype(np.float64) if d is not None else np.zeros(shape)
        full = full[..., mask]
        if m is None:
            return full
        if len(m) and np.all(m == m[0]):
            return full[:, :, :int(m[0])], bins
        return [full[:, f, :int(m[f])] for f in range(shape[1])], bins

    def doppler_azimuth_peaks_device(self, proc, rx_sets, groups, range_windows, shift_angle=True, precise_vel_ranges=None,
                                     min_threshold_dB=30.0):
        """``doppler_azimuth_device`` and then ``mmw_doppler_azimuth_peaks`` on the maps it left in HBM; only the two index tables
        are downloaded: ``(row_peak, zero, m, bins)`` with ``row_peak`` int32 ``[G, F, rows]`` (the column among the valid angle
        bins of each row's peak), ``zero`` int32 ``[G, F]`` (the row of the zero-azimuth peak); -1: none, -2: undecided.
        ``self.dopaz_peak_maps`` keeps ``(buffer, shape)`` of the maps for the frames the host has to pick again."""
        # every argument check comes before the first use of self.ctx / self.bufs
        n_sets = max(len(rx_sets), 1)
        shift = np.atleast_1d(np.asarray(shift_angle, dtype=bool))
        if shift.shape == (1,):
            shift = np.repeat(shift, n_sets)
        if shift.shape != (n_sets,):
            raise ValueError(f"doppler_azimuth: shift_angle must be a bool or one per set ({n_sets}), got {shift.shape}")
        table = _peak_groups(groups, n_sets, shift)
        thr = float(min_threshold_dB)
        if not (np.isfinite(thr) and thr >= 0.0):
            raise ValueError(f"doppler_azimuth_peaks: min_threshold_dB must be finite and non-negative, got {min_threshold_dB}")
        valid = np.flatnonzero(np.asarray(getattr(proc, "valid_angle_mask", True), dtype=bool))   # another proc: refused below
        if valid.size == 0 or not np.array_equal(valid, np.arange(valid[0], valid[-1] + 1)):
            raise ValueError("doppler_azimuth_peaks: the valid angle bins must be one non-empty run of columns")
        d, shape, m, bins = self.doppler_azimuth_device(proc, rx_sets, range_windows, shift_angle, precise_vel_ranges)
        _, F, n_rows, A = shape
        G = len(table)
        row_peak = np.full((G, F, n_rows), _lib.DOPAZ_PEAK_NONE, dtype=np.int32)
        zero = np.full((G, F), _lib.DOPAZ_PEAK_NONE, dtype=np.int32)
        self.dopaz_peak_maps = (d, shape)
        if d is None or G == 0:
            return row_peak, zero, m, bins
        a_lo, a_hi = int(valid[0]), int(valid[-1]) + 1
        a_zero = a_lo + int(np.argmin(np.abs(proc.valid_angle_bins)))
        d_row = self.bufs.get("dopaz_row_peak", row_peak.nbytes)
        d_zero = self.bufs.get("dopaz_zero_peak", zero.nbytes)
        ip = lambda a: a.ctypes.data_as(_lib._ip)      # noqa: E731
        h_m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
        _lib.check(self.ctx.lib.mmw_doppler_azimuth_peaks(self.ctx.handle, d.ptr, shape[0], F, n_rows, A, ip(table), G,
                                                          None if h_m is None else ip(h_m), a_lo, a_hi, a_zero, thr, 4.0,
                                                          d_row.ptr, d_zero.ptr))
        return d_row.download(row_peak.shape, np.int32), d_zero.download(zero.shape, np.int32), m, bins

    def doppler_azimuth_peaks(self, proc, rx_sets, groups, range_windows, shift_angle=True, precise_vel_ranges=None,
                              min_threshold_dB=30.0):
        """The peak pickers of the reference's Doppler-azimuth velocity loop (processors/velocity_estimator.py:785-865) on the maps
        of ``doppler_azimuth``, picked on the device: ``(row_peaks, zero_az)`` with ``row_peaks[g][f]`` what
        ``proc.detect_peaks_rows(map, vel_bins, min_threshold_dB)`` returns for frame f's map of ``groups[g]`` -- one set's map, or
        the mean of two sets' maps (``(resp_1 + resp_2) / 2``) -- and ``zero_az[g][f]`` what ``proc.detect_peak_zero_az`` returns;
        ``vel_bins`` are ``proc.vel_bins``, or the frame's ``zoomed_vel_bins`` with ``precise_vel_ranges``.

        ``groups``: per group a set index, ``(set,)`` or ``(set, set)`` into ``rx_sets``; two sets must share ``shift_angle``.
        Frames the device left undecided (a comparison inside ``MMW_DOPAZ_PEAK_BAND``, a non-finite map such as that of an empty
        range window) are picked by the host pickers from that frame's downloaded maps; ``self.n_peaks_undecided`` counts them
        per (group, frame).  A precise frame without velocity bins yields empty results.  The other arguments are those of
        ``doppler_azimuth``; ``proc`` is only read."""
        row_peak, zero, m, bins = self.doppler_azimuth_peaks_device(proc, rx_sets, groups, range_windows, shift_angle,
                                                                    precise_vel_ranges, min_threshold_dB)
        d, shape = self.dopaz_peak_maps
        G, F, n_rows = row_peak.shape
        valid_bins = np.asarray(proc.valid_angle_bins, dtype=np.float64)
        mask = np.asarray(proc.valid_angle_mask, dtype=bool)
        if m is None:
            rows_of = np.full(F, n_rows, dtype=np.int64)
            vel = np.broadcast_to(np.asarray(proc.vel_bins, dtype=np.float64), (F, n_rows))
        else:
            rows_of = np.asarray(m, dtype=np.int64)
            vel = np.zeros((F, n_rows))
            for f in range(F):
                vel[f, :rows_of[f]] = bins[f]
        # every decided peak of the batch at once, then cut into its (group, frame) pieces
        found = row_peak >= 0
        _, f_idx, r_idx = np.nonzero(found)
        pairs = np.stack([valid_bins[row_peak[found]], vel[f_idx, r_idx]], axis=1)
        pieces = np.split(pairs, np.cumsum(found.sum(axis=2).ravel())[:-1]) if G * F else []
        undecided = (np.any(row_peak == _lib.DOPAZ_PEAK_UNDECIDED, axis=2) | (zero == _lib.DOPAZ_PEAK_UNDECIDED)) & (rows_of > 0)[None, :]
        table = _peak_groups(groups, shape[0], np.zeros(shape[0], dtype=bool))
        row_peaks, zero_az = [], []
        for g in range(G):
            row_peaks.append([])
            zero_az.append([])
            for f in range(F):
                if undecided[g, f]:
                    frame_bytes = n_rows * shape[3] * 4
                    sets = [d.download((n_rows, shape[3]), np.float32, (int(k) * F + f) * frame_bytes).astype(np.float64)
                            for k in table[g] if k >= 0]
                    resp = (sets[0] if len(sets) == 1 else (sets[0] + sets[1]) / 2)[:rows_of[f], mask]
                    row_peaks[g].append(proc.detect_peaks_rows(resp, vel[f, :rows_of[f]], min_threshold_dB))
                    zero_az[g].append(proc.detect_peak_zero_az(resp, vel[f, :rows_of[f]], min_threshold_dB))
                    continue
                row_peaks[g].append(pieces[g * F + f])
                z = int(zero[g, f])
                zero_az[g].append(np.array([0.0, vel[f, z]]) if z >= 0 else np.empty(shape=(0, 2)))
        self.n_peaks_undecided = int(undecided.sum())
        return row_peaks, zero_az

    def doppler_azimuth_fits(self, estimator, altitudes, enable_precise_responses=False):
        """Stages 1 to 3 of ``processors.velocity_estimator.VelocityEstimator.process`` (the ADC-cube path) for every resident
        frame: ``(fits [F, G, 4], status [F, G])`` with ``fits[f, g] = (vx, vy, R^2, inlier share)`` of group g (0: azimuth,
        1: elevation on an ods array) and ``status`` one of ``_lib.DOPAZ_STATUS_OK / _EMPTY / _FAILED`` -- what ``dopaz_state_scan``
        turns into the estimator's track.  Range windows, antenna sets, valid angle columns, the peak threshold and the gates are
        read from the estimator as ``process`` derives them; ``altitudes``: one per frame, or one for all.

        The maps, the peak picker and ``mmw_doppler_azimuth_ransac`` run on the device, the regression on the index tables the
        picker left in HBM.  With ``enable_precise_responses`` the coarse pass gives vx, ``precise_ranges_from_zero_az`` the
        velocity ranges, and the precise maps, picker and fit follow (the reference's order).  A pair the kernel flagged is
        refitted by the estimator's own scikit-learn function from that pair's peaks (picked again by the host pickers from the
        frame's downloaded maps where its tables held a -2); ``self.n_dopaz_fits_flagged`` counts them.  ``x_measurement_only``
        estimators run the zero-azimuth part only.  The estimator is only read."""
        import copy
        from .point_cloud_processing import ransac_tables
        from .processors import velocity_estimator as ve
        # every argument check comes before the first use of self.ctx / self.bufs
        if not isinstance(estimator, ve.VelocityEstimator):
            raise ValueError("doppler_azimuth_fits: estimator must be a processors.velocity_estimator.VelocityEstimator, got "
                             f"{type(estimator).__name__}")
        F = self.n_frames
        alt = np.asarray(altitudes, dtype=np.float64)
        if alt.ndim == 0:
            alt = np.full(F, float(alt))
        if alt.shape != (F,) or not np.all(np.isfinite(alt)):
            raise ValueError(f"doppler_azimuth_fits: altitudes must be {F} finite numbers (one per resident frame) or one, got "
                             f"shape {alt.shape}")
        gates = (float(estimator.min_R2_threshold), float(estimator.min_inlier_percent))
        if not np.all(np.isfinite(gates)):
            raise ValueError(f"doppler_azimuth_fits: the estimator's gates must be finite, got {gates}")
        cm = estimator.config_manager
        sets, groups, shift = ve.antenna_plan(cm)
        G = len(groups)
        windows = np.stack([estimator.get_range_window(altitude=a, sensing_direction=cm.array_direction) for a in alt]) \
            if F else np.zeros((0, 2))
        thr_dB = estimator.peak_threshold_dB
        theta = np.ascontiguousarray(estimator.valid_angle_bins, dtype=np.float64)
        mode = _lib.DOPAZ_RANSAC_VX_ONLY if estimator.x_measurement_only else 0
        pv = None
        if enable_precise_responses:
            _, zero_az = self.doppler_azimuth_peaks(estimator, sets, groups, windows, shift, None, thr_dB)
            pv = precise_ranges_from_zero_az(zero_az[0], zero_az[1] if G == 2 else None, estimator.precise_vel_bound)
        row_peak, zero, m, bins = self.doppler_azimuth_peaks_device(estimator, sets, groups, windows, shift, pv, thr_dB)
        d, shape = self.dopaz_peak_maps
        n_rows = row_peak.shape[2]
        fits = np.zeros((F, G, 4))
        status = np.full((F, G), _lib.DOPAZ_STATUS_EMPTY, dtype=np.int32)
        self.n_dopaz_fits_flagged = 0
        if F == 0:
            return fits, status
        if m is None:
            rows_of = np.full(F, n_rows, dtype=np.int64)
            vel = np.ascontiguousarray(estimator.vel_bins, dtype=np.float64)
            vel_of = lambda f: vel                      # noqa: E731
        else:
            rows_of = np.asarray(m, dtype=np.int64)
            vel = np.zeros((F, max(n_rows, 1)))
            for f in range(F):
                vel[f, :rows_of[f]] = bins[f]
            vel_of = lambda f: vel[f]                   # noqa: E731
        flags = np.zeros((G, F), dtype=np.int32)
        if d is not None and n_rows > 0:
            subsets, trials = ransac_tables.dopaz_tables(n_rows)
            key = ("dopaz_ransac_tables", n_rows)
            if getattr(self, "_dopaz_ransac_key", None) != key:          # uploaded once per n_rows and kept
                self.bufs.get("dopaz_ransac_subsets", subsets.nbytes).upload(subsets)
                self.bufs.get("dopaz_ransac_trials", trials.nbytes).upload(trials)
                self._dopaz_ransac_key = key
            d_sub = self.bufs.get("dopaz_ransac_subsets", subsets.nbytes)
            d_tri = self.bufs.get("dopaz_ransac_trials", trials.nbytes)
            angles = np.ascontiguousarray(np.stack([np.cos(theta), np.sin(theta), theta]))
            d_ang = self.bufs.get("dopaz_ransac_angles", angles.nbytes)
            if getattr(self, "_dopaz_ransac_angles", None) != angles.tobytes():   # they change with the estimator only
                d_ang.upload(angles)
                self._dopaz_ransac_angles = angles.tobytes()
            d_vel = self.bufs.get("dopaz_ransac_vel", vel.nbytes)
            d_vel.upload(vel)
            d_row = self.bufs.get("dopaz_row_peak", row_peak.nbytes)
            d_zero = self.bufs.get("dopaz_zero_peak", zero.nbytes)
            d_out = self.bufs.get("dopaz_ransac_out", G * F * 32)
            d_flags = self.bufs.get("dopaz_ransac_flags", G * F * 4)
            h_m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
            nc = len(theta)
            _lib.check(self.ctx.lib.mmw_doppler_azimuth_ransac(
                self.ctx.handle, d_row.ptr, d_zero.ptr, G, F, n_rows, None if h_m is None else h_m.ctypes.data_as(_lib._ip),
                d_vel.ptr, vel.shape[-1], int(vel.ndim == 2), d_ang.ptr, d_ang.at(nc * 8), d_ang.at(2 * nc * 8), nc, d_sub.ptr,
                d_tri.ptr, max(n_rows - ransac_tables.MIN_SAMPLES + 1, 0), len(trials), 0, 1 if G == 2 else -1, mode,
                ve.THRESHOLD_STANDARD, ve.THRESHOLD_SMALL_VX, gates[0], gates[1], d_out.ptr, d_flags.ptr))
            fits = d_out.download((G, F, 4), np.float64).transpose(1, 0, 2).copy()
            flags = d_flags.download((G, F), np.int32).copy()
            status = ((flags >> _lib.DOPAZ_STATUS_SHIFT) & _lib.DOPAZ_STATUS_MASK).T.astype(np.int32)
        # pairs the device left to the host: the frame's peaks (picked again where a table entry is undecided), the class's fit
        redo = (flags & _lib.DOPAZ_FLAG_MASK) != 0           # no maps (a batch without velocity rows): every pair is empty
        self.n_dopaz_fits_flagged = int(redo.sum())
        if redo.any():
            table = _peak_groups(groups, shape[0], np.zeros(shape[0], dtype=bool))
            mask = np.asarray(estimator.valid_angle_mask, dtype=bool)
            tmp = copy.copy(estimator)
            for f in np.flatnonzero(redo.any(axis=0)):
                mf, v = int(rows_of[f]), vel_of(f)
                picked = []
                for g in range(G):
                    if d is not None and (np.any(row_peak[g, f, :mf] == _lib.DOPAZ_PEAK_UNDECIDED) or zero[g, f] == _lib.DOPAZ_PEAK_UNDECIDED):
                        frame_bytes = n_rows * shape[3] * 4
                        maps = [d.download((n_rows, shape[3]), np.float32, (int(k) * F + f) * frame_bytes).astype(np.float64)
                                for k in table[g] if k >= 0]
                        resp = (maps[0] if len(maps) == 1 else (maps[0] + maps[1]) / 2)[:mf, mask]
                        picked.append((estimator.detect_peaks_rows(resp, v[:mf], thr_dB), estimator.detect_peak_zero_az(resp, v[:mf], thr_dB)))
                    else:
                        rows = np.flatnonzero(row_peak[g, f, :mf] >= 0)
                        z = int(zero[g, f])
                        picked.append((np.stack([theta[row_peak[g, f, rows]], v[rows]], axis=1),
                                       np.array([0.0, v[z]]) if z >= 0 else np.empty(shape=(0, 2))))
                tmp.azimuth_peak_zero_az = picked[0][1]
                tmp.elevation_peak_zero_az = picked[1][1] if G == 2 else np.empty(shape=(0, 2))
                vx = tmp.estimate_ego_vx_velocity()
                for g in np.flatnonzero(redo[:, f]):
                    peaks = picked[g][0]
                    if mode or peaks.shape[0] == 0:
                        fits[f, g] = (vx, 0.0, 0.0, 0.0)
                        status[f, g] = _lib.DOPAZ_STATUS_OK if mode else _lib.DOPAZ_STATUS_EMPTY
                        continue
                    fit = tmp.lsq_fit_ego_vy_ransac(peaks=peaks)
                    fits[f, g] = (vx,) + tuple(fit)
                    status[f, g] = _lib.DOPAZ_STATUS_FAILED if tuple(fit) == (0.0, 0.0, 0.0) else _lib.DOPAZ_STATUS_OK
        return fits, status

    def doppler_azimuth_velocities(self, estimator, altitudes, enable_precise_responses=False) -> np.ndarray:
        """``estimator.process(adc_cube=cube_f, altitude=altitudes[f], enable_precise_responses=...)`` of every resident frame in
        order: ``[F, 3]`` current estimates.  ``doppler_azimuth_fits`` and then ``dopaz_state_scan``, which advances the estimator
        (its state carries across calls and ``stream()`` chunks)."""
        fits, status = self.doppler_azimuth_fits(estimator, altitudes, enable_precise_responses)
        return dopaz_state_scan(estimator, fits, status)

    def synthetic_array_device(self, proc, velocities) -> Tuple[np.ndarray, _lib.DeviceBuffer]:
        """``(frames, buffer)``: the images of ``synthetic_array`` left in HBM, complex64 ``[n_valid][S][n_az * n_el]``, nothing
        downloaded."""
        # every argument check comes before the first use of self.ctx / self.bufs
        v, frames, P, dirs, _, _ = self._synthetic_array_arguments(proc, velocities, "synthetic_array")
        T, H, k = dirs.shape[1], int(proc.num_frames), int(proc.stride)
        self.d_synth = self.bufs.get("synth_array", max(len(frames), 1) * self.S * T * 8)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(self.ctx.lib.mmw_synth_array(self.ctx.handle, self.d_in.ptr, self.n_frames, self.V, self.S, self.C, v,
                                                k, H, frames.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(frames),
                                                P.ctypes.data_as(dp), dirs.ctypes.data_as(dp), T, float(proc.lambda_m),
                                                self.d_synth.ptr))
        return frames.astype(np.int64), self.d_synth

    def synthetic_array(self, proc, velocities) -> Tuple[np.ndarray, np.ndarray]:
        """``(frames, responses)``: ``responses[i]`` (complex128 ``[n_valid, S, n_az, n_el]``) is what a fresh
        ``SyntheticArrayBeamformerProcessor`` configured like ``proc`` returns for resident frame ``frames[i]`` when it is stepped
        through the resident frames with ``velocities [n_frames, 3]``; ``frames`` are the frames whose geometry is valid (the
        others return ``np.empty(0)`` there).  One ``mmw_synth_array`` call: the window of every valid frame (``num_frames``
        frames of every ``stride``-th chirp of virtual antenna ``chirp_cfg_idx * num_rx + receiver_idx``) is read in place from
        the resident cubes, the geometry table comes from ``synthetic_array_geometry``.  ``proc`` is not touched.  Works on
        whatever ``load`` / ``load_raw`` / ``load_raw_i16`` / ``synth`` left resident.
        Out of scope: carrying the ``num_frames - 1`` frames of history across ``stream()`` chunks or calls (every call starts
        from a reset history), and ``MultiDeviceFramePipeline`` (a shard needs a halo of ``num_frames - 1`` frames)."""
        frames, d = self.synthetic_array_device(proc, velocities)
        n_az, n_el = np.shape(proc.d)[1:]
        out = d.download((len(frames), self.S, n_az * n_el), np.complex64) if len(frames) else np.zeros((0, self.S, n_az * n_el), np.complex64)
        return frames, out.astype(np.complex128).reshape(len(frames), self.S, n_az, n_el)

    def _synthetic_array_arguments(self, proc, velocities, what: str):
        """The argument checks of ``synthetic_array*`` (no device use) -> ``(v, frames, P, dirs, n_az, n_el)``."""
        if getattr(proc, "enable_calibration", False):
            raise ValueError(f"{what}: array calibration is not part of this build")
        cm = proc.config_manager
        num_tx = int(cm.frameCfg_end_index) - int(cm.frameCfg_start_index) + 1
        if self.V % num_tx or self.S != proc.num_range_bins or self.C * num_tx != proc.chirps_per_frame:
            raise ValueError(f"{what}: cubes [{self.V}, {self.S}, {self.C}] do not match the processor's configuration "
                             f"({num_tx} transmitters, {proc.num_range_bins} samples, {proc.chirps_per_frame} chirps per frame)")
        num_rx = self.V // num_tx
        rx, tx = int(proc.receiver_idx), int(proc.chirp_cfg_idx) - int(cm.frameCfg_start_index)
        if not (0 <= rx < num_rx and 0 <= tx < num_tx):
            raise ValueError(f"{what}: receiver {rx} / chirp configuration {proc.chirp_cfg_idx} is not one of {num_rx} "
                             f"receivers x {num_tx} transmitters")
        vel = np.asarray(velocities, dtype=np.float64)
        if vel.shape != (self.n_frames, 3):
            raise ValueError(f"{what}: velocities must be [{self.n_frames}, 3] (one row per resident frame), got {vel.shape}")
        valid, P = synthetic_array_geometry(proc, vel)
        frames = np.flatnonzero(valid).astype(np.int32)
        n_az, n_el = (int(n) for n in np.shape(proc.d)[1:])
        dirs = np.ascontiguousarray(np.asarray(proc.d, dtype=np.float64).reshape(3, -1))
        return tx * num_rx + rx, frames, np.ascontiguousarray(P), dirs, n_az, n_el

    def synthetic_array_calibrated_device(self, proc, velocities, num_calibration_iters: int = 1) -> Tuple[np.ndarray, _lib.DeviceBuffer]:
        """``(frames, buffer)``: the images of ``synthetic_array_calibrated`` left in HBM, complex64 ``[n_valid][S][n_az * n_el]``.
        Kept on the pipeline: ``synth_geometry_calibrated [n_valid, 3, E]``, ``synth_calib_status [n_valid]`` (iterations that
        applied a correction), ``synth_calib_targets [n_valid, 3, 2]`` (range row, azimuth bin; -1: none) and ``n_flagged``."""
        # every argument check comes before the first use of self.ctx / self.bufs
        n_it = int(num_calibration_iters)
        if not 1 <= n_it <= 8:
            raise ValueError(f"synthetic_array_calibrated: num_calibration_iters {num_calibration_iters} is not in [1, 8]")
        v, frames, P, dirs, n_az, n_el = self._synthetic_array_arguments(proc, velocities, "synthetic_array_calibrated")
        T, H, k, n = n_az * n_el, int(proc.num_frames), int(proc.stride), len(frames)
        E, lam = P.shape[2], float(proc.lambda_m)
        self._synth_calib_key = None
        self.d_synth = self.bufs.get("synth_array", max(n, 1) * self.S * T * 8)
        d_P = self.bufs.get("synth_calib_P", max(n, 1) * 3 * E * 8)
        d_st = self.bufs.get("synth_calib_status", max(n, 1) * 4)
        d_tg = self.bufs.get("synth_calib_targets", max(n, 1) * 24)
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        lib, h = self.ctx.lib, self.ctx.handle
        _lib.check(lib.mmw_synth_array_calibrate(h, self.d_in.ptr, self.n_frames, self.V, self.S, self.C, v, k, H,
                                                 frames.ctypes.data_as(ip), n, P.ctypes.data_as(dp), dirs.ctypes.data_as(dp), n_az, n_el,
                                                 lam, n_it, self.d_synth.ptr, d_P.ptr, d_st.ptr, d_tg.ptr))
        if n:
            Pcal, status = d_P.download((n, 3, E), np.float64), d_st.download((n,), np.int32)
            targets = d_tg.download((n, 3, 2), np.int32)
        else:
            Pcal, status, targets = np.zeros((0, 3, E)), np.zeros(0, np.int32), np.zeros((0, 3, 2), np.int32)
        flagged = np.flatnonzero(status < 0)
        self.n_flagged = len(flagged)
        if len(flagged):
            # the host route: calibrate_window per flagged frame, its contractions as ONE mmw_synth_array call per round over the
            # frames still in the loop (scratch buffer), then one call with the final geometries into the frames' own slots
            fl_frames = np.ascontiguousarray(frames[flagged])
            d_tmp = self.bufs.get("synth_calib_flagged", len(flagged) * self.S * T * 8)

            def contract_all(geoms):
                g = np.ascontiguousarray(geoms)
                _lib.check(lib.mmw_synth_array(h, self.d_in.ptr, self.n_frames, self.V, self.S, self.C, v, k, H,
                                               fl_frames.ctypes.data_as(ip), len(fl_frames), g.ctypes.data_as(dp),
                                               dirs.ctypes.data_as(dp), T, lam, d_tmp.ptr))
                out = d_tmp.download((len(fl_frames), self.S, T), np.complex64)
                return out.astype(np.complex128).reshape(len(fl_frames), self.S, n_az, n_el)

            Cv, slab = E // H, self.S * self.C * 8
            windows = []
            for f in fl_frames:
                w = np.zeros((H, self.S, Cv), dtype=complex)
                for hh in range(H):
                    fr = int(f) - H + 1 + hh
                    if fr >= 0:
                        w[hh] = self.d_in.download((self.S, self.C), np.complex64, byte_offset=(fr * self.V + v) * slab)[:, ::k]
                windows.append(w.transpose(1, 0, 2).reshape(self.S, E))
            geoms = P[flagged].copy()                # geometry of the latest image of every flagged frame
            imgs = contract_all(geoms)
            state = [dict(status=0, targets=[], Pcal=P[q].copy(), live=True) for q in flagged]
            from .processors.synthetic_array_beamformer import calibration_spectra, calibration_targets, calibrated_geometry
            spectra = [calibration_spectra(w) for w in windows]
            for _ in range(n_it):
                moved = False
                for j, q in enumerate(flagged):
                    st = state[j]
                    if not st["live"]:
                        continue
                    tg = calibration_targets(spectra[j], imgs[j])
                    if len(tg) < 3:
                        st["live"], st["Pcal"] = False, P[q].copy()
                        continue
                    st["Pcal"] = calibrated_geometry(spectra[j], P[q], tg, np.asarray(proc.d, dtype=np.float64), lam)
                    geoms[j], st["targets"], st["status"], moved = st["Pcal"], tg, st["status"] + 1, True
                if not moved:
                    break
                imgs = contract_all(geoms)
            for j, q in enumerate(flagged):
                Pcal[q], status[q] = state[j]["Pcal"], state[j]["status"]
                targets[q] = -1
                for t, rc in enumerate(state[j]["targets"]):
                    targets[q, t] = rc
            # the final images of the flagged frames, into their slots of the result
            out = d_tmp.download((len(fl_frames), self.S, T), np.complex64)
            for j, q in enumerate(flagged):
                self.d_synth.upload(out[j], byte_offset=int(q) * self.S * T * 8)
        self.synth_geometry_calibrated, self.synth_calib_status, self.synth_calib_targets = Pcal, status, targets
        # for synthetic_array_patterns(calibrated=True): what was calibrated, and the rows of d_P the host route has since corrected
        self._synth_calib_key = (v, k, H, lam, n_it, n_az, n_el, frames, P, dirs)
        self._synth_calib_stale = [int(q) for q in flagged]
        return frames.astype(np.int64), self.d_synth

    def synthetic_array_calibrated(self, proc, velocities, num_calibration_iters: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """``(frames, responses)``: what a fresh ``SelfCalibratingSyntheticArrayProcessor`` configured like ``proc`` (a plain
        ``SyntheticArrayBeamformerProcessor``, only read) returns for the valid resident frames: complex128 ``[n_valid, S, n_az,
        n_el]``.  One ``mmw_synth_array_calibrate`` call: uncalibrated images, the calibration loop and the calibrated images are
        enqueued together; frames whose discrete decisions the device cannot take for certain (``n_flagged`` of them) are
        calibrated on the host from their downloaded windows and contracted again.  Fewer than three range peaks or a window
        slot before the buffer give "no suitable targets" (status 0) where the reference raises ``IndexError``.  Scope as
        ``synthetic_array``: no history across ``stream()`` chunks, no ``MultiDeviceFramePipeline``."""
        frames, d = self.synthetic_array_calibrated_device(proc, velocities, num_calibration_iters)
        n_az, n_el = np.shape(proc.d)[1:]
        out = d.download((len(frames), self.S, n_az * n_el), np.complex64) if len(frames) else np.zeros((0, self.S, n_az * n_el), np.complex64)
        return frames, out.astype(np.complex128).reshape(len(frames), self.S, n_az, n_el)

    def synthetic_array_patterns_device(self, proc, velocities, calibrated: bool = False,
                                        num_calibration_iters: int = 1) -> Tuple[np.ndarray, _lib.DeviceBuffer]:
        """``(frames, buffer)``: the patterns of ``synthetic_array_patterns`` left in HBM, float32 ``[n_valid][n_az * n_el]``,
        nothing downloaded."""
        # every argument check comes before the first use of self.ctx / self.bufs
        what = "synthetic_array_patterns"
        if calibrated:
            n_it = int(num_calibration_iters)
            if not 1 <= n_it <= 8:
                raise ValueError(f"{what}: num_calibration_iters {num_calibration_iters} is not in [1, 8]")
            v, frames, P, dirs, n_az, n_el = self._synthetic_array_arguments(proc, velocities, what)
        else:
            valid, P = synthetic_array_geometry(proc, velocities)
            frames = np.flatnonzero(valid)
        P, d, lam = array_pattern_args(P, proc.d, proc.lambda_m, what)
        n, E, T = P.shape[0], P.shape[2], d.shape[1] * d.shape[2]
        if calibrated:
            # the geometries are read where mmw_synth_array_calibrate left them; only rows the host route corrected are uploaded
            key = (v, int(proc.stride), int(proc.num_frames), lam, n_it, n_az, n_el, frames, P, dirs)
            have = self._synth_calib_key
            if have is None or not all(np.array_equal(a, b) for a, b in zip(have, key)):
                self.synthetic_array_calibrated_device(proc, velocities, n_it)
            d_P = self.bufs.get("synth_calib_P", max(n, 1) * 3 * E * 8)
            for q in self._synth_calib_stale:
                d_P.upload(self.synth_geometry_calibrated[q], byte_offset=q * 3 * E * 8)
            self._synth_calib_stale = []
        else:
            d_P = self.bufs.get("synth_pattern_P", max(n, 1) * 3 * E * 8)
            if n:
                d_P.upload(P)
        self.d_synth_pattern = self.bufs.get("synth_pattern", max(n, 1) * T * 4)
        array_patterns_on(self.ctx, d_P.ptr, n, E, d, lam, self.d_synth_pattern)
        return frames.astype(np.int64), self.d_synth_pattern

    def synthetic_array_patterns(self, proc, velocities, calibrated: bool = False,
                                 num_calibration_iters: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """``(frames, patterns)``: the beam pattern float32 ``[n_valid, n_az, n_el]`` of every valid frame's synthetic array (the
        reference's ``compute_synthetic_array_pattern``: ``|sum_e exp(j 2 pi d . p_e / lambda)|`` over the steering grid,
        normalised per frame), one ``mmw_synth_array_pattern`` call on this pipeline's context.  ``calibrated=False``: the
        geometries of ``synthetic_array_geometry`` -- ``batch.synthetic_array_patterns``; no cubes are read and ``velocities``
        may have any number of rows.  ``calibrated=True``: the geometries ``synthetic_array_calibrated_device(proc, velocities,
        num_calibration_iters)`` produced (``synth_geometry_calibrated``), read in place from its device buffer; the calibration
        is run first unless its results for these arguments and the resident cubes are still there.  Scope as
        ``synthetic_array``."""
        frames, buf = self.synthetic_array_patterns_device(proc, velocities, calibrated, num_calibration_iters)
        n_az, n_el = np.shape(proc.d)[1:]
        out = buf.download((len(frames), n_az, n_el), np.float32) if len(frames) else np.zeros((0, n_az, n_el), np.float32)
        return frames, out

    def _alloc_detect(self):
        F, V, cap = self.n_frames, self.V, self.cap
        self.d_rd = self.bufs.get("rd", max(F, 1) * self.cube_bytes)
        self.d_dets = self.bufs.get("dets", max(F, 1) * cap * 8)
        self.d_cnt = self.bufs.get("counts", max(F, 1) * 4)
        self.d_l1 = self.bufs.get("plane_l1", max(F, 1) * V * 4)     # error-bound scale (CFAR screening, exact argmax)

    def _cfar_args(self):
        (tr, td), (gr, gd) = self.cfar.num_train, self.cfar.num_guard
        return self.cfar.kind, int(tr), int(td), int(gr), int(gd), float(self.cfar._scale()), int(self.cfar._k_rank())

    def _detect_float64(self, f0: int, nf: int):
        """The float64 path for frames [f0, f0 + nf): RD + float64 |RD| of antenna 0 + CFAR + ordered compaction."""
        V, S, C, cap = self.V, self.S, self.C, self.cap
        n = S * C
        d_mag = self.bufs.get("mag64", max(self.n_frames, 1) * n * 8)
        d_mask = self.bufs.get("mask", max(self.n_frames, 1) * n)
        kind, tr, td, gr, gd, scale, k_rank = self._cfar_args()
        _lib.check(self.ctx.lib.mmw_detect_batch(self.ctx.handle, self.d_in.at(f0 * self.cube_bytes), self.d_rd.at(f0 * self.cube_bytes),
                                                 d_mag.at(f0 * n * 8), d_mask.at(f0 * n), self.d_dets.at(f0 * cap * 8),
                                                 self.d_cnt.at(f0 * 4), self.d_l1.at(f0 * V * 4), nf, V, S, C, kind, tr, td, gr, gd,
                                                 scale, k_rank, cap))

    def _detect_integrated(self, f0: int, nf: int):
        """``_detect_float64`` with the power summed over ``integrate_rx`` as the CFAR plane (``mmw_detect_batch_integrated``)."""
        V, S, C, cap = self.V, self.S, self.C, self.cap
        n = S * C
        self.d_pow = self.bufs.get("pow64", max(self.n_frames, 1) * n * 8)
        d_mask = self.bufs.get("mask", max(self.n_frames, 1) * n)
        kind, tr, td, gr, gd, scale, k_rank = self._cfar_args()
        ants, n_ants = _lib.int_array(self.integrate_rx)
        _lib.check(self.ctx.lib.mmw_detect_batch_integrated(
            self.ctx.handle, self.d_in.at(f0 * self.cube_bytes), self.d_rd.at(f0 * self.cube_bytes), self.d_pow.at(f0 * n * 8),
            d_mask.at(f0 * n), self.d_dets.at(f0 * cap * 8), self.d_cnt.at(f0 * 4), self.d_l1.at(f0 * V * 4), nf, V, S, C, kind,
            tr, td, gr, gd, scale, k_rank, cap, ants, n_ants))

    def integrated_power_device(self) -> _lib.DeviceBuffer:
        """The CFAR plane of ``integrate_rx=``: float64 ``[F, S, C]`` in HBM, ``sum_v |RD_v|^2`` over the listed antennas in list
        order (``mmw_range_doppler_power64``), computed from the resident cubes by this call."""
        if self.integrate_rx is None:
            raise ValueError("integrated_power: the pipeline was built without integrate_rx=")
        F, n = self.n_frames, self.S * self.C
        self.d_pow = self.bufs.get("pow64", max(F, 1) * n * 8)
        ants, n_ants = _lib.int_array(self.integrate_rx)
        for f0 in range(0, F, 32768):
            _lib.check(self.ctx.lib.mmw_range_doppler_power64(self.ctx.handle, self.d_in.at(f0 * self.cube_bytes),
                                                              self.d_pow.at(f0 * n * 8), min(32768, F - f0), self.V, self.S,
                                                              self.C, ants, n_ants))
        return self.d_pow

    def integrated_power(self, lo: int = 0, hi: Optional[int] = None) -> np.ndarray:
        """Frames ``[lo, hi)`` of ``integrated_power_device()`` on the host, float64 ``[hi - lo, S, C]``."""
        buf = self.integrated_power_device()
        lo, hi, _ = slice(lo, hi).indices(self.n_frames)
        n = self.S * self.C
        if hi <= lo:
            return np.zeros((0, self.S, self.C))
        return buf.download((hi - lo, self.S, self.C), np.float64, lo * n * 8)

    def _argmax_float64(self, d_idx, ant, shift, f0: int, nf: int):
        cap = self.cap
        arr, n_ant = _lib.int_array(ant)
        n_ref = _lib.C.c_int(0)
        if self.tdm_compensation:
            table = tdm_phase_table(ant, self.tdm_slots[0], self.tdm_slots[1], self.C)
            _lib.check(self.ctx.lib.mmw_angle_argmax_tdm(self.ctx.handle, self.d_in.at(f0 * self.cube_bytes), self.d_l1.at(f0 * self.V * 4),
                                                         self.d_rd.at(f0 * self.cube_bytes), self.d_dets.at(f0 * cap * 8),
                                                         self.d_cnt.at(f0 * 4), d_idx.at(f0 * cap * 4), nf, self.V, self.S, self.C,
                                                         cap, arr, n_ant, self.A, int(shift), table.ctypes.data, _lib.C.byref(n_ref)))
            self.n_refined += n_ref.value
            return
        _lib.check(self.ctx.lib.mmw_angle_argmax_exact(self.ctx.handle, self.d_in.at(f0 * self.cube_bytes), self.d_l1.at(f0 * self.V * 4),
                                                       self.d_rd.at(f0 * self.cube_bytes), self.d_dets.at(f0 * cap * 8),
                                                       self.d_cnt.at(f0 * 4), d_idx.at(f0 * cap * 4), nf, self.V, self.S, self.C,
                                                       cap, arr, n_ant, self.A, int(shift), _lib.C.byref(n_ref)))
        self.n_refined += n_ref.value

    def _argmax_hypotheses(self):
        """``tdm_velocity_unwrap=True``: the deciding list through ``mmw_angle_argmax_tdm_hyp`` (every hypothesis; ``d_hyp`` gets the
        choice), the other list(s) through the same entry with the hypothesis given."""
        F, cap = self.n_frames, self.cap
        which, deciding = self.tdm_hyp_list
        slots, n_slots = self.tdm_slots
        self.d_hyp = self.bufs.get("tdm_hyp", max(F, 1) * cap * 4)
        lists = {"az": (self.az, self.shift_az, "az_idx"), "el": (self.el, self.shift_el, "el_idx"),
                 "list": (deciding, False, "tdm_hyp_idx")}
        out = {}
        for key in (which,) + tuple(k for k in ("az", "el") if k != which):
            ant, shift, name = lists[key]
            if not ant:
                out[key] = None
                continue
            d_idx = out[key] = self.bufs.get(name, max(F, 1) * cap * 4)
            arr, n_ant = _lib.int_array(ant)
            table = tdm_hypothesis_table(ant, slots, n_slots, self.C)
            for f0 in range(0, F, 32768):
                n_ref = _lib.C.c_int(0)
                _lib.check(self.ctx.lib.mmw_angle_argmax_tdm_hyp(
                    self.ctx.handle, self.d_in.at(f0 * self.cube_bytes), self.d_l1.at(f0 * self.V * 4), self.d_rd.at(f0 * self.cube_bytes),
                    self.d_dets.at(f0 * cap * 8), self.d_cnt.at(f0 * 4), d_idx.at(f0 * cap * 4), self.d_hyp.at(f0 * cap * 4),
                    int(key != which), min(32768, F - f0), self.V, self.S, self.C, cap, arr, n_ant, self.A, int(shift),
                    table.ctypes.data, n_slots, _lib.C.byref(n_ref)))
                self.n_refined += n_ref.value
        self.d_az, self.d_el = out["az"], out["el"]

    def _tdm_hyp_host(self) -> np.ndarray:
        """``d_hyp`` on the host, ``[F, cap]`` int32, the slots past a frame's count zeroed."""
        if not self.tdm_velocity_unwrap or self.__dict__.get("d_hyp") is None:
            raise ValueError("tdm_hypotheses: needs tdm_velocity_unwrap=True and a point-cloud call on the resident frames")
        hyp = self.d_hyp.download((self.n_frames, self.cap), np.int32).copy()
        hyp[np.arange(self.cap)[None, :] >= np.clip(self.counts, 0, self.cap)[:, None]] = 0
        return hyp

    def tdm_hypotheses(self, lo: int = 0, hi: Optional[int] = None) -> np.ndarray:
        """The velocity hypothesis ``h*`` of every detection of frames ``[lo, hi)`` after a point-cloud call with
        ``tdm_velocity_unwrap=True``: int32 ``[hi - lo, cap]``, frame f's ``counts[f]`` detections first, zeros behind them."""
        hyp = self._tdm_hyp_host()
        lo, hi, _ = slice(lo, hi).indices(self.n_frames)
        return hyp[lo:max(hi, lo)]

    def tdm_unwrapped_bins(self, lo: int = 0, hi: Optional[int] = None) -> np.ndarray:
        """The unwrapped Doppler bins ``k' = sym(k + h* C)`` of the same detections (``tdm_unwrapped_bin``): int64 ``[hi - lo, cap]``,
        zeros behind a frame's detections."""
        hyp = self._tdm_hyp_host()
        lo, hi, _ = slice(lo, hi).indices(self.n_frames)
        hi = max(hi, lo)
        cols = self.d_dets.download((self.n_frames, self.cap, 2), np.int32)[lo:hi, :, 1]
        out = tdm_unwrapped_bin(cols, hyp[lo:hi], self.tdm_slots[1], self.C)
        out[np.arange(self.cap)[None, :] >= np.clip(self.counts[lo:hi], 0, self.cap)[:, None]] = 0
        return out

    def _fused_supported(self, with_angles: bool) -> bool:
        kind, tr, td, gr, gd, _, _ = self._cfar_args()
        n_az, n_el = (len(self.az), len(self.el)) if with_angles else (0, 0)
        return bool(self.ctx.lib.mmw_detect_points_supported(self.S, self.C, kind, tr, td, gr, gd, n_az, n_el, self.A))

    def _detect_fused(self, with_angles: bool):
        """``mmw_detect_points``: RD + screened CFAR (undecided cells settled in float64) + ordered compaction (+ the
        azimuth / elevation argmax bins) in one pass; frames it hands back (count -1) go through the float64 path."""
        F, V, S, C, cap = self.n_frames, self.V, self.S, self.C, self.cap
        kind, tr, td, gr, gd, scale, k_rank = self._cfar_args()
        az, n_az = _lib.int_array(self.az if with_angles else [])
        el, n_el = _lib.int_array(self.el if with_angles else [])
        self.d_az = self.bufs.get("az_idx", max(F, 1) * cap * 4) if n_az else None
        self.d_el = self.bufs.get("el_idx", max(F, 1) * cap * 4) if n_el else None
        stats = (_lib.C.c_int * 5)()
        self.screen_stats = np.zeros(5, dtype=np.int64)
        step = max(1, min(F, (2 ** 31 - 1) // max(cap, 1)))
        for f0 in range(0, F, step):
            nf = min(step, F - f0)
            _lib.check(self.ctx.lib.mmw_detect_points(
                self.ctx.handle, self.d_in.at(f0 * self.cube_bytes), self.d_rd.at(f0 * self.cube_bytes), self.d_l1.at(f0 * V * 4),
                None, self.d_dets.at(f0 * cap * 8), self.d_cnt.at(f0 * 4), self.d_az.at(f0 * cap * 4) if n_az else None,
                self.d_el.at(f0 * cap * 4) if n_el else None, nf, V, S, C, kind, tr, td, gr, gd, scale, k_rank, cap,
                az, n_az, int(self.shift_az), el, n_el, int(self.shift_el), self.A, stats))
            self.screen_stats += np.array(list(stats), dtype=np.int64)
        self.n_refined += int(self.screen_stats[3] + self.screen_stats[4])
        counts = self.d_cnt.download((F,), np.int32)
        for f in np.nonzero(counts < 0)[0]:            # not decidable by the screening pass: the float64 path, frame by frame
            self._detect_float64(int(f), 1)
            if n_az:
                self._argmax_float64(self.d_az, self.az, self.shift_az, int(f), 1)
            if n_el:
                self._argmax_float64(self.d_el, self.el, self.shift_el, int(f), 1)
        if np.any(counts < 0):
            counts = self.d_cnt.download((F,), np.int32)
        return counts

    def _check_capacity(self, counts) -> None:
        self.counts = counts
        if np.any(counts > self.cap):
            raise _lib.MmwGpuError(f"detection capacity {self.cap} exceeded (max count {int(counts.max())}): "
                                   "raise det_capacity")

    def _fetch_dets(self, counts) -> List[np.ndarray]:
        F, cap = self.n_frames, self.cap
        self._check_capacity(counts)
        dets = self.d_dets.download((F, cap, 2), np.int32)
        self.dets = [dets[f, :counts[f]].astype(np.int64) for f in range(F)]
        return self.dets

    # ------------------------------------------------------------------ ground detector
    def _ground_picks(self, d_cand, d_cnt, shape, host_pick) -> Tuple[np.ndarray, np.ndarray]:
        """Candidate table + counts of a device picker; entries it flagged (count -1) are re-picked by ``host_pick(index)``,
        which returns the candidate ranges RangeProcessor.find_peaks gives on the data the device left behind."""
        cand = d_cand.download(shape, np.float64).copy()
        cnt = d_cnt.download(shape[:-1], np.int32).copy()
        for idx in zip(*(i.tolist() for i in np.nonzero(cnt < 0))):
            got = host_pick(idx)
            cand[idx][:len(got)] = got
            cnt[idx] = len(got)
            self.n_flagged += 1
        return cand, cnt

    def _detect_ground(self) -> np.ndarray:
        """RD (+ L1 norms) and float64 |RD| of antenna 0 for every frame; range-profile peaks (and the zoom peaks around every
        one of them) on the device; the Altimeter's scan over the frames on the host; the gated Doppler CFAR + ordered
        compaction on the device.  Returns the detection counts."""
        F, V, S, C, cap = self.n_frames, self.V, self.S, self.C, self.cap
        L, h, bufs = self.ctx.lib, self.ctx.handle, self.bufs
        det = self.ground
        alt, vel = det.altimeter, det.vel_detector
        precise = bool(det.altimeter_params.get("precise_est_enabled", True))
        F1 = max(F, 1)
        d_mag = bufs.get("mag64", F1 * S * C * 8)
        d_prof, d_bins = bufs.get("g_profile", F1 * S * 8), bufs.get("g_bins", S * 8)
        d_cand, d_ccnt = bufs.get("g_cand", F1 * 3 * 8), bufs.get("g_ccount", F1 * 4)
        d_bins.upload(np.ascontiguousarray(alt.range_bins[:S], dtype=np.float64))
        self.n_flagged = 0
        step = 32768
        for f0 in range(0, F, step):
            nf = min(step, F - f0)
            cube = self.d_in.at(f0 * self.cube_bytes)
            _lib.check(L.mmw_range_doppler(h, cube, self.d_rd.at(f0 * self.cube_bytes), None, nf, V, S, C))
            _lib.check(L.mmw_plane_l1(h, cube, self.d_l1.at(f0 * V * 4), nf, V, S, C))
            _lib.check(L.mmw_range_doppler_mag64(h, cube, d_mag.at(f0 * S * C * 8), nf, V, S, C, 0))
            _lib.check(L.mmw_ground_candidates(h, cube, d_bins.ptr, d_prof.at(f0 * S * 8), d_cand.at(f0 * 24), d_ccnt.at(f0 * 4),
                                               nf, V, S, C))

        def coarse_pick(idx):
            prof = d_prof.download((S,), np.float64, idx[0] * S * 8)
            return alt.find_peaks(20 * np.log10(prof), alt.range_bins, max_peaks=3)[0]
        cand, ccnt = self._ground_picks(d_cand, d_ccnt, (F, 3), coarse_pick)
        coarse = [cand[f, :ccnt[f]].tolist() for f in range(F)]
        fine = None
        if precise:
            half = float(alt.zoom_half_width_m)
            hi_cap = float(alt.range_bins.max()) - 1e-6
            d_spec = bufs.get("g_spec", F1 * 3 * S * 8)
            d_zc, d_zcnt = bufs.get("g_zcand", F1 * 6 * 8), bufs.get("g_zcount", F1 * 3 * 4)
            if self.n_flagged:                              # the host's picks replace the flagged rows
                d_cand.upload(cand)
                d_ccnt.upload(ccnt)
            for f0 in range(0, F, step):
                nf = min(step, F - f0)
                _lib.check(L.mmw_ground_zoom_candidates(h, self.d_in.at(f0 * self.cube_bytes), d_cand.at(f0 * 24), d_ccnt.at(f0 * 4),
                                                        d_spec.at(f0 * 3 * S * 8), d_zc.at(f0 * 48), d_zcnt.at(f0 * 12), nf,
                                                        V, S, C, half, hi_cap, 1 / self.cm.range_res_m, float(self.cm.range_max_m)))

            def zoom_pick(idx):
                f, j = idx
                c = cand[f, j]
                lo, hi = max(1e-6, c - half), min(hi_cap, c + half)          # Altimeter._look_zoom's window
                spec = d_spec.download((S,), np.float64, (f * 3 + j) * S * 8)
                return alt.find_peaks(20 * np.log10(spec), np.linspace(lo, hi, S), max_peaks=2)[0]
            zc, zcnt = self._ground_picks(d_zc, d_zcnt, (F, 3, 2), zoom_pick)
            fine = [[zc[f, j, :zcnt[f, j]].tolist() for j in range(3)] for f in range(F)]
        self._scan_inputs = (coarse, fine)                  # (kept for tools/ground_batch_probe.py's timing of the scan)
        self.altitudes = np.array(alt.lock.advance(coarse, fine), dtype=np.float64)
        d_gate = bufs.get("g_gate", F1 * 8)
        d_gate.upload(ground_gates(det.range_bins, self.altitudes))
        d_mask = bufs.get("mask", F1 * S * C)
        for f0 in range(0, F, step):
            nf = min(step, F - f0)
            _lib.check(L.mmw_cfar1d_gated(h, d_mag.at(f0 * S * C * 8), d_gate.at(f0 * 8), d_mask.at(f0 * S * C),
                                          self.d_dets.at(f0 * cap * 8), self.d_cnt.at(f0 * 4), nf, S, C, int(vel.kind),
                                          int(vel.num_train), int(vel.num_guard), float(vel._scale()), int(vel._k_rank()), cap))
        return self.d_cnt.download((F,), np.int32)

    # ------------------------------------------------------------------ sequential detector
    def _detect_sequential(self, with_rd: bool) -> np.ndarray:
        """Float64 chirp-0 range profiles -> range CFAR -> row lists (``mmw_seq_rows``), then the Doppler rows of the listed
        range bins, the velocity CFAR and the ordered hits in one kernel (``mmw_seq_detect``; ``mmw_seq_detect_plane`` when
        ``mmw_seq_route`` says so).  ``with_rd``: also the float32 RD cube and the plane norms the exact argmax reads
        (``point_clouds()``); ``detect()`` alone needs neither and skips both.  Returns the detection counts."""
        F, V, S, C, cap = self.n_frames, self.V, self.S, self.C, self.cap
        L, h, bufs = self.ctx.lib, self.ctx.handle, self.bufs
        rng, vel = _cfar1d_args(self.sequential.rng_detector), _cfar1d_args(self.sequential.vel_detector)
        F1 = max(F, 1)
        d_prof = bufs.get("s_profile", F1 * S * 8)
        d_rows, d_nrows = bufs.get("s_rows", F1 * S * 4), bufs.get("s_nrows", F1 * 4)
        plane = bool(L.mmw_seq_route(h, S, C))
        if plane:
            d_mag, d_mask = bufs.get("mag64", F1 * S * C * 8), bufs.get("mask", F1 * S * C)
        step = 32768                        # grid limits of the per-frame launches
        for f0 in range(0, F, step):
            nf = min(step, F - f0)
            cube = self.d_in.at(f0 * self.cube_bytes)
            if with_rd:
                _lib.check(L.mmw_range_doppler(h, cube, self.d_rd.at(f0 * self.cube_bytes), None, nf, V, S, C))
                _lib.check(L.mmw_plane_l1(h, cube, self.d_l1.at(f0 * V * 4), nf, V, S, C))
            _lib.check(L.mmw_range_profile_f64(h, cube, d_prof.at(f0 * S * 8), nf, V, S, C, 0))
            rows, nrows = d_rows.at(f0 * S * 4), d_nrows.at(f0 * 4)
            _lib.check(L.mmw_seq_rows(h, d_prof.at(f0 * S * 8), rows, nrows, nf, S, *rng))
            dets, cnt = self.d_dets.at(f0 * cap * 8), self.d_cnt.at(f0 * 4)
            if plane:
                _lib.check(L.mmw_seq_detect_plane(h, cube, rows, nrows, d_mag.at(f0 * S * C * 8), d_mask.at(f0 * S * C), dets, cnt,
                                                  nf, V, S, C, *vel, cap))
            else:
                _lib.check(L.mmw_seq_detect(h, cube, rows, nrows, dets, cnt, nf, V, S, C, *vel, cap, None))
        return self.d_cnt.download((F,), np.int32)

    def detect(self) -> List[np.ndarray]:
        """RD (all antennas, fp32) + CFAR on antenna 0 (with ``integrate_rx=``: on the power summed over the listed antennas) +
        ordered compaction for every frame.

        Returns the per-frame int64 ``(N, 2)`` [range_idx, doppler_idx] arrays (row-major order, == np.where).  With
        ``ground=``: the ground detector's detections (gated rows, Doppler CFAR), and ``altitudes`` is set.  With
        ``sequential=``: the sequential detector's detections; the float32 RD cube is not computed (``point_clouds()``
        computes it for the argmax)."""
        self._alloc_detect()
        return self._fetch_dets(self._detect_counts())

    def _detect_counts(self) -> np.ndarray:
        """The detections of ``detect()`` left on the device (``d_dets`` / ``d_cnt``); returns the counts."""
        F = self.n_frames
        if self.ground is not None:
            return self._detect_ground()
        if self.sequential is not None:
            return self._detect_sequential(False)
        if self.integrate_rx is not None:
            for f0 in range(0, F, 32768):
                self._detect_integrated(f0, min(32768, F - f0))
            return self.d_cnt.download((F,), np.int32)
        if self._fused_supported(False):
            return self._detect_fused(False)
        for f0 in range(0, F, 32768):       # grid limits of the per-frame launches
            self._detect_float64(f0, min(32768, F - f0))
        return self.d_cnt.download((F,), np.int32)

    def _argmax_device(self, ant, shift, name) -> _lib.DeviceBuffer:
        """Exact (float64-equivalent) argmax bins of every detection, ``[F, cap]`` int32 on the device: ``mmw_angle_argmax_exact``
        (``tdm_compensation=True``: ``mmw_angle_argmax_tdm``)."""
        F, cap = self.n_frames, self.cap
        d_idx = self.bufs.get(name, max(F, 1) * cap * 4)
        for f0 in range(0, F, 32768):
            self._argmax_float64(d_idx, ant, shift, f0, min(32768, F - f0))
        return d_idx

    def _detect_points(self, fetch: bool) -> np.ndarray:
        """Detections and their angle bins for every frame, left on the device (``d_dets``, ``d_cnt``, ``d_az``, ``d_el``; an
        empty antenna list leaves None).  ``fetch``: also the host lists of ``detect()`` (``self.dets``).  Returns the counts."""
        self.n_refined = 0      # detections re-evaluated in float64 (near-ties of the float32 pass)
        self._alloc_detect()
        if (self.ground is None and self.sequential is None and self.integrate_rx is None and not self.tdm_compensation
                and self._fused_supported(True)):
            counts = self._detect_fused(True)
            self._fetch_dets(counts) if fetch else self._check_capacity(counts)
            return counts
        counts = self._detect_sequential(True) if self.sequential is not None else self._detect_counts()
        self._fetch_dets(counts) if fetch else self._check_capacity(counts)
        if self.tdm_velocity_unwrap:
            self._argmax_hypotheses()
            return counts
        self.d_az = self._argmax_device(self.az, self.shift_az, "az_idx") if self.az else None
        self.d_el = self._argmax_device(self.el, self.shift_el, "el_idx") if self.el else None
        return counts

    def point_clouds(self) -> List[np.ndarray]:
        """Per-frame float64 ``(N, 4)`` (x, y, z, velocity), FLU frame (point_cloud_generator.py:216-248)."""
        F, cap = self.n_frames, self.cap
        self._detect_points(True)
        dets = self.dets
        az_idx = self.d_az.download((F, cap), np.int32) if self.az else None
        el_idx = self.d_el.download((F, cap), np.int32) if self.el else None
        if self.tdm_velocity_unwrap:
            hyp, span = self.d_hyp.download((F, cap), np.int32), 2.0 * self.cm.vel_max_m_s
        out = []
        for f, d in enumerate(dets):
            n = d.shape[0]
            if n == 0:
                out.append(np.empty((0, 4)))
                continue
            az = self.angle_bins[az_idx[f, :n]] if az_idx is not None else np.zeros(n)
            el = self.angle_bins[el_idx[f, :n]] if el_idx is not None else np.zeros(n)
            rng, vel = self.range_bins[d[:, 0]], self.vel_bins[d[:, 1]]
            if self.tdm_velocity_unwrap:        # v + m span where the chosen hypothesis folds; m == 0 keeps the table's bits
                k = d[:, 1] - self.C // 2
                m = (tdm_unwrapped_bin(d[:, 1], hyp[f, :n], self.tdm_slots[1], self.C) - k) // self.C
                vel = np.where(m != 0, vel + m.astype(np.float64) * span, vel)
            cos_el = np.cos(el)
            out.append(np.column_stack((rng * cos_el * np.cos(az), rng * cos_el * np.sin(az), rng * np.sin(el), vel)))
        self.az_idx = None if az_idx is None else [az_idx[f, :len(d)].astype(np.int64) for f, d in enumerate(dets)]
        self.el_idx = None if el_idx is None else [el_idx[f, :len(d)].astype(np.int64) for f, d in enumerate(dets)]
        return out

    # ------------------------------------------------------------------ device point clouds, ego velocity
    def point_clouds_device(self) -> _lib.DeviceBuffer:
        """``point_clouds()`` without the download and the per-frame host loop: a packed float64 ``[F, cap, 4]`` (x, y, z,
        velocity) buffer in HBM (``mmw_point_cloud``), frame f holding its ``counts[f]`` points first and zeros behind them.
        ``fetch_point_clouds()`` downloads it to the lists ``point_clouds()`` returns, bit for bit."""
        F, cap = self.n_frames, self.cap
        self._detect_points(False)
        tabs = self.__dict__.get("_pc_tables")
        if tabs is None:                    # float64 tables made on the host (no device libm), uploaded once
            tabs = tuple(self.bufs.get(f"pc_tab{i}", t.nbytes) for i, t in enumerate(
                (self.range_bins, self.vel_bins, np.cos(self.angle_bins), np.sin(self.angle_bins))))
            for buf, t in zip(tabs, (self.range_bins, self.vel_bins, np.cos(self.angle_bins), np.sin(self.angle_bins))):
                buf.upload(np.ascontiguousarray(t, dtype=np.float64))
            self._pc_tables = tabs
        self.d_points = self.bufs.get("points", max(F, 1) * cap * 32)
        d_az, d_el = (self.d_az if self.az else None), (self.d_el if self.el else None)
        for f0 in range(0, F, 32768):
            _lib.check(self.ctx.lib.mmw_point_cloud(
                self.ctx.handle, self.d_dets.at(f0 * cap * 8), self.d_cnt.at(f0 * 4), d_az.at(f0 * cap * 4) if d_az else None,
                d_el.at(f0 * cap * 4) if d_el else None, tabs[0].ptr, tabs[1].ptr, tabs[2].ptr, tabs[3].ptr,
                self.d_points.at(f0 * cap * 32), min(32768, F - f0), cap, len(self.range_bins), len(self.vel_bins), self.A))
            if self.tdm_velocity_unwrap:
                _lib.check(self.ctx.lib.mmw_tdm_unwrap_velocity(
                    self.ctx.handle, self.d_points.at(f0 * cap * 32), self.d_dets.at(f0 * cap * 8), self.d_cnt.at(f0 * 4),
                    self.d_hyp.at(f0 * cap * 4), min(32768, F - f0), cap, self.C, self.tdm_slots[1],
                    2.0 * self.cm.vel_max_m_s))
        self._points_cnt = self.d_cnt
        return self.d_points

    def fetch_point_clouds(self) -> List[np.ndarray]:
        """The buffer of ``point_clouds_device()`` as per-frame ``(N, 4)`` arrays."""
        pts = self.d_points.download((self.n_frames, self.cap, 4), np.float64)
        return [pts[f, :n] if n else np.empty((0, 4)) for f, n in enumerate(self.counts)]

    def _upload_points(self, point_clouds: Sequence[np.ndarray]) -> Tuple[int, np.ndarray]:
        """Caller-made point clouds in place of the detector's: packed into the ``[F, cap, 4]`` buffer (the loaded cubes and
        their detections are left alone).  Returns the frame count and the point counts."""
        F, cap = len(point_clouds), self.cap
        if F > self.max_frames:
            raise ValueError("more point clouds than max_frames")
        counts = np.array([len(p) for p in point_clouds], dtype=np.int32)
        if np.any(counts > cap):
            raise _lib.MmwGpuError(f"a point cloud of {int(counts.max())} points exceeds det_capacity {cap}")
        packed = np.zeros((max(F, 1), cap, 4))
        for f, p in enumerate(point_clouds):
            if len(p):
                packed[f, :len(p)] = np.asarray(p, dtype=np.float64).reshape(-1, 4)
        self.d_points = self.bufs.get("points", max(F, 1) * cap * 32)
        self.d_points.upload(packed)
        self._points_cnt = self.bufs.get("points_cnt", max(F, 1) * 4)
        self._points_cnt.upload(counts)
        return F, counts

    def ego_fits(self, estimator, point_clouds: Optional[Sequence[np.ndarray]] = None, with_mask: bool = False):
        """The per-frame RANSAC fits of ``estimator`` for every frame (``mmw_ego_velocity_ransac``): float64 ``[F, dim + 2]``
        rows (coefficients, R^2 on the inliers, inlier share), dim = 2 for the ``standard`` array geometry and 3 for ``ods``;
        zeros where the fit fails.  Frames the kernel flags (``ego_flags``, ``n_ego_flagged``: a decision within rounding of
        scikit-learn's) are recomputed by the estimator's own scikit-learn fit.  Point clouds: those of
        ``point_clouds_device()``, or the caller's ``point_clouds`` (``(N, 4)`` arrays).  Returns (fits, counts)."""
        from .point_cloud_processing import ransac_tables as T
        from .point_cloud_processing.vel_estimator import RESIDUAL_THRESHOLD
        from .point_cloud_processing.vel_estimator import GEOMETRY_DIM
        geometry = estimator.config_manager.array_geometry
        if geometry not in GEOMETRY_DIM:
            raise ValueError(f"ego velocity needs the standard or the ods array geometry, not {geometry!r}")
        dim = GEOMETRY_DIM[geometry]
        if point_clouds is None:
            self.point_clouds_device()
            F, counts = self.n_frames, self.counts
        else:
            F, counts = self._upload_points(point_clouds)
        cap = self.cap
        subsets, row, tab, offs = T.frame_tables(counts)
        bufs, F1 = self.bufs, max(F, 1)
        d_sub, d_row = bufs.get("ego_subsets", max(subsets.nbytes, 16)), bufs.get("ego_row", F1 * 4)
        d_tab, d_off = bufs.get("ego_trials", tab.nbytes), bufs.get("ego_trials_off", max(offs.nbytes, 16))
        for buf, arr in ((d_sub, subsets), (d_row, row), (d_tab, tab), (d_off, offs)):
            if arr.size:
                buf.upload(arr)
        d_out, d_flags = bufs.get("ego_out", F1 * (dim + 2) * 8), bufs.get("ego_flags", F1 * 4)
        d_mask = bufs.get("ego_mask", F1 * cap) if with_mask else None
        for f0 in range(0, F, 32768):
            _lib.check(self.ctx.lib.mmw_ego_velocity_ransac(
                self.ctx.handle, self.d_points.at(f0 * cap * 32), self._points_cnt.at(f0 * 4), min(32768, F - f0), cap, dim,
                RESIDUAL_THRESHOLD, float(estimator.min_R2_threshold), d_sub.ptr, d_row.at(f0 * 4), len(offs), d_tab.ptr, len(tab),
                d_off.ptr, d_out.at(f0 * (dim + 2) * 8), d_flags.at(f0 * 4), d_mask.at(f0 * cap) if with_mask else None))
        fits = d_out.download((F, dim + 2), np.float64).copy()
        self.ego_flags = d_flags.download((F,), np.int32).copy()
        self.ego_masks = d_mask.download((F, cap), np.uint8).copy().astype(bool) if with_mask else None
        flagged = np.nonzero(self.ego_flags)[0]
        self.n_ego_flagged = len(flagged)
        fit = estimator.lsq_fit_ego_vel_ransac_points_2D if dim == 2 else estimator.lsq_fit_ego_vel_ransac_points_3D
        for f in flagged.tolist():              # within rounding of a decision: scikit-learn itself decides
            n = int(counts[f])
            pts = self.d_points.download((n, 4), np.float64, f * cap * 32)
            if with_mask:
                from .point_cloud_processing.vel_estimator import ransac_fit
                coef, r2, share, mask = ransac_fit(pts, dim, return_mask=True)
                self.ego_masks[f, :n] = mask
            else:
                coef, r2, share = fit(points=pts)
            fits[f] = 0.0
            fits[f, :len(coef)] = coef
            fits[f, dim:] = r2, share
        return fits, counts

    def ego_velocities(self, estimator, point_clouds: Optional[Sequence[np.ndarray]] = None) -> np.ndarray:
        """``estimator.process(points=...)`` (a ``VelocityEstimator``) called on every frame's point cloud in order: float64
        ``[F, 3]`` current velocity estimates.  The fits run on the device (``ego_fits``); the estimator's state (statistics,
        proposal, current estimate) is advanced frame by frame on the host and carries across calls and ``stream()`` chunks."""
        fits, counts = self.ego_fits(estimator, point_clouds)
        return ego_state_scan(estimator, fits, counts)

    # ------------------------------------------------------------------ vehicle velocity RANSAC
    def vehicle_fits(self, estimator, point_clouds: Optional[Sequence[np.ndarray]] = None, initial=None, track: bool = False,
                     only_2D: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """``estimator.estimate_ego_vel`` (a ``VehicleVelEstimator``) for every frame (``mmw_vehicle_velocity_ransac``): float64
        ``[F, dim + 2]`` rows (ego velocity, mean squared error of the winning refit, points behind the static filter) and int32
        ``status [F]`` (1: an estimate; 0: the class's empty array, the row's velocity and error zero), dim = 2 for ``only_2D``.
        Point clouds: those of ``point_clouds_device()``, or the caller's ``point_clouds`` (``(N, 4)`` arrays).  ``initial``: None,
        or ``[F, dim]`` previous estimates for the static filter, a NaN row for a frame that has none.  ``track=True``: the
        frames form one drive -- each takes the last estimate found before it as its initial estimate (``initial``: None or
        the ``[dim]`` estimate before the first frame) -- which runs as ONE workgroup walking the frames in order.  Frames the
        kernel flags (``vehicle_flags``, ``n_vehicle_flagged``: a decision within rounding of the host class's) are recomputed by
        the estimator's host path with the same draws; a chain goes on behind such a frame from the recomputed estimate.  The
        draws' seed is ``estimator.seed``, or, when that is None, one drawn from OS entropy for this call (``vehicle_seed``).
        The estimator itself is left untouched."""
        import copy
        import os
        from .point_cloud_processing import ransac_tables as T
        dim = 2 if only_2D else 3
        ppf, iters, ncp = int(estimator.points_per_fit), int(estimator.max_iters), int(estimator.num_close_pts)
        n_init = None if point_clouds is None else len(point_clouds)
        F_known = self.n_frames if n_init is None else n_init
        init = None
        if initial is not None:
            init = np.ascontiguousarray(initial, dtype=np.float64)
            want = (dim,) if track else (F_known, dim)
            if init.shape != want:
                raise ValueError(f"vehicle_fits: initial must have shape {want}{' with track=True' if track else ''}, got {init.shape}")
        if point_clouds is None:
            self.point_clouds_device()
            F, counts = self.n_frames, np.asarray(self.counts)
        else:
            F, counts = self._upload_points(point_clouds)
        cap, bufs, F1 = self.cap, self.bufs, max(F, 1)
        seed = estimator.seed if estimator.seed is not None else int.from_bytes(os.urandom(8), "little")
        self.vehicle_seed = seed
        live = counts[counts >= ncp]
        n_max = int(live.max()) if live.size else 0
        filtered = track or (init is not None and not np.isnan(init).any(axis=-1).all())
        draws = T.vehicle_tables(seed, range(ncp, n_max + 1) if filtered else live.tolist(), n_max, iters, ppf)
        d_draws = bufs.get("vehicle_draws", draws.nbytes)
        d_draws.upload(draws)
        d_out, d_status, d_flags = (bufs.get("vehicle_out", F1 * (dim + 2) * 8), bufs.get("vehicle_status", F1 * 4),
                                    bufs.get("vehicle_flags", F1 * 4))
        d_init = bufs.get("vehicle_init", F1 * dim * 8)
        host = copy.copy(estimator)

        def launch(f0, n, has_init, chain):
            _lib.check(self.ctx.lib.mmw_vehicle_velocity_ransac(
                self.ctx.handle, self.d_points.at(f0 * cap * 32), self._points_cnt.at(f0 * 4), n, cap, dim, ppf, iters,
                float(estimator.fit_thresh), ncp, float(estimator.static_vel_thresh), d_init.ptr if has_init else None, d_draws.ptr,
                len(draws), int(chain), d_out.at(f0 * (dim + 2) * 8), d_status.at(f0 * 4), d_flags.at(f0 * 4)))

        def fetch(f0, n):
            return (d_out.download((n, dim + 2), np.float64, f0 * (dim + 2) * 8).copy(),
                    d_status.download((n,), np.int32, f0 * 4).copy(), d_flags.download((n,), np.int32, f0 * 4).copy())

        def on_host(f, prior):
            """Frame f by the estimator's host path: its row and status."""
            pts = self.d_points.download((int(counts[f]), 4), np.float64, f * cap * 32) if counts[f] else np.empty((0, 4))
            have = prior is not None and not np.isnan(prior).any()
            found, kept = host.ransac(pts, prior if have else np.empty(0), only_2D, seed=seed)
            row = np.zeros(dim + 2)
            if found:
                row[:dim], row[dim] = host.get_vehicle_vel_est(), host.best_error
            row[dim + 1] = kept
            return row, int(found)

        if not track:
            if init is not None and F:
                d_init.upload(init)
            launch(0, F, init is not None, False)
            fits, status, flags = fetch(0, F) if F else (np.zeros((0, dim + 2)), np.zeros(0, np.int32), np.zeros(0, np.int32))
            for f in np.nonzero(flags)[0].tolist():
                fits[f], status[f] = on_host(f, None if init is None else init[f])
        else:
            fits, status, flags = np.zeros((F, dim + 2)), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32)
            carry = None if init is None or np.isnan(init).any() else init.copy()
            f0 = 0
            while f0 < F:
                if carry is not None:
                    d_init.upload(carry)
                launch(f0, F - f0, carry is not None, True)
                out, st, fl = fetch(f0, F - f0)
                stop = int(np.nonzero(fl)[0][0]) if fl.any() else F - f0
                fits[f0:f0 + stop], status[f0:f0 + stop] = out[:stop], st[:stop]
                found = np.nonzero(st[:stop])[0]
                if len(found):
                    carry = out[found[-1], :dim].copy()
                f0 += stop
                if f0 < F:                      # the frame that ended the chain: the host decides it, the chain goes on behind it
                    flags[f0] = fl[stop]
                    fits[f0], status[f0] = on_host(f0, carry)
                    if status[f0]:
                        carry = fits[f0, :dim].copy()
                    f0 += 1
        self.vehicle_flags = flags
        self.n_vehicle_flagged = int(np.count_nonzero(flags))
        return fits, status

    def vehicle_velocities(self, estimator, point_clouds: Optional[Sequence[np.ndarray]] = None, initial=None, track: bool = False,
                           only_2D: bool = True) -> np.ndarray:
        """``estimator.estimate_ego_vel`` on every frame in order (``vehicle_fits``): float64 ``[F, dim]``, a NaN row where the
        class returns the empty array.  ``estimator.best_fit`` and ``estimator.best_error`` are left as the frame loop leaves them."""
        fits, status = self.vehicle_fits(estimator, point_clouds, initial, track, only_2D)
        return vehicle_state_scan(estimator, fits, status)


def vehicle_state_scan(estimator, fits: np.ndarray, status: np.ndarray) -> np.ndarray:
    """The ``[F, dim]`` estimates (NaN rows: none) of ``vehicle_fits``' rows, and the state ``VehicleVelEstimator.estimate_ego_vel``
    leaves behind frame by frame: nothing changes below ``num_close_pts`` points, the error is reset to inf from there on, and a
    found estimate installs its fit (minus the velocity) and its error."""
    dim = fits.shape[1] - 2
    out = np.full((len(fits), dim), np.nan)
    for f in range(len(fits)):
        if fits[f, dim + 1] < estimator.num_close_pts:
            continue
        if status[f]:
            out[f] = fits[f, :dim]
            estimator.best_fit, estimator.best_error = -1 * fits[f, :dim], float(fits[f, dim])
        else:
            estimator.best_error = np.inf
    return out


def ego_state_scan(estimator, fits: np.ndarray, counts: Sequence[int]) -> np.ndarray:
    """``VelocityEstimator.process`` for every frame given the frames' fits (``[F, dim + 2]``) and point counts: an empty frame
    leaves the statistics and the proposal of the last non-empty one in place, and every frame ends in the estimator's
    threshold check.  A failed fit (inlier share 0) proposes what the estimator's fit functions return for it: zeros, a
    2-vector under the ``ods`` geometry too."""
    dim = fits.shape[1] - 2
    out = np.empty((len(counts), 3))
    for f, n in enumerate(counts):
        if n > 0:
            share = fits[f, dim + 1]
            estimator.take_fit(dim, (fits[f, :dim].copy() if share > 0 else np.zeros(2), float(fits[f, dim]), share))
        estimator.update_and_check_current_vel_measurements()
        out[f] = estimator.current_velocity_estimate
    return out


def dopaz_state_scan(estimator, fits: np.ndarray, status: np.ndarray) -> np.ndarray:
    """Advance a ``processors.velocity_estimator.VelocityEstimator`` over the frames of ``FramePipeline.doppler_azimuth_fits``:
    ``fits [F, G, 4]`` (vx, vy, R^2, share), ``status [F, G]``; returns the ``[F, 3]`` current estimates, as stepping
    ``process(adc_cube=...)`` frame by frame would.  An empty group keeps the fit its direction had (the class fits only
    directions with row peaks), a failed fit installs zeros, the proposal is formed in the geometry's component order and the
    gates are the class's own.  The estimator's state carries over to the next call."""
    fits = np.asarray(fits, dtype=np.float64)
    status = np.asarray(status)
    if fits.ndim != 3 or fits.shape[2] != 4 or status.shape != fits.shape[:2]:
        raise ValueError(f"dopaz_state_scan: fits must be [F, G, 4] and status [F, G], got {fits.shape} and {status.shape}")
    geometry = estimator.config_manager.array_geometry
    G = {"standard": 1, "ods": 2}.get(geometry)
    if G is None or fits.shape[1] != G:
        raise ValueError(f"dopaz_state_scan: a {geometry} array has {G} groups, the fits hold {fits.shape[1]}")
    out = np.zeros((len(fits), 3))
    for f in range(len(fits)):
        estimator.ego_vx_estimate = float(fits[f, 0, 0])
        took = [None if status[f, g] == _lib.DOPAZ_STATUS_EMPTY else
                ((0.0, 0.0, 0.0) if status[f, g] == _lib.DOPAZ_STATUS_FAILED else tuple(float(x) for x in fits[f, g, 1:]))
                for g in range(G)]
        if estimator.x_measurement_only:
            took = []
        estimator.take_fits(*took)
        estimator.update_and_check_current_vel_measurements()
        out[f] = estimator.current_velocity_estimate
    return out


class MultiDeviceFramePipeline:
    """One process, every visible device: the frame range is block-split (``shard_bounds``) over one ``FramePipeline``
    per device, each driven by its own host thread (a context is only ever touched by its thread), results land in
    disjoint slices of caller-owned arrays and per-frame lists come back concatenated in frame order.  No device
    talks to another (no collective).  This is what the reference's single-process frame loops
    (scripts/test_vel_estimation.py:145-151) turn into on a multi-GPU node; ``bench.py --gpus N`` keeps the
    one-process-per-GPU form.

    The ground detector (``FramePipeline(ground=...)``) is refused: its Altimeter carries an altitude track from each frame
    to the next, which a split by frames would break.  ``sequential=`` has no state across frames and shards like ``cfar=``.

    ``part_factory(device, max_frames)`` builds the per-device pipeline (default: ``FramePipeline`` on a new
    ``Context(device)``); tests inject a host-only fake to exercise the split / join logic without a GPU."""

    def __init__(self, config_manager, max_frames: int, shape: Tuple[int, int, int], devices: Optional[Sequence[int]] = None,
                 part_factory: Optional[Callable[[int, int], object]] = None, **pipeline_kwargs):
        from concurrent.futures import ThreadPoolExecutor
        if pipeline_kwargs.get("ground") is not None:
            raise ValueError("MultiDeviceFramePipeline cannot take ground=: the altitude track runs through the frames in "
                             "order, so it cannot be split across devices -- use one FramePipeline(ground=...)")
        if devices is None:
            devices = list(range(_lib.device_count()))
        self.devices = [int(d) for d in devices]
        if not self.devices:
            raise _lib.MmwGpuError("no HIP device visible: the MI355X HIP path is the only backend")
        self.world = len(self.devices)
        self.max_frames = int(max_frames)
        self.shape = tuple(int(x) for x in shape)
        per_dev = -(-self.max_frames // self.world)
        if part_factory is None:
            def part_factory(device, n):
                return FramePipeline(config_manager, n, shape, ctx=_lib.Context(device), **pipeline_kwargs)
        # one single-thread executor per device: every call on a device's context comes from the same host thread
        self._pools = [ThreadPoolExecutor(max_workers=1, thread_name_prefix=f"mmw-dev{d}") for d in self.devices]
        self.parts = self._each(lambda r: part_factory(self.devices[r], per_dev), all_ranks=True)
        self.n_frames = 0
        self.bounds: List[Tuple[int, int]] = [(0, 0)] * self.world

    # ------------------------------------------------------------------ plumbing
    def _each(self, fn, all_ranks: bool = False) -> List:
        """``fn(rank)`` on every device thread that holds frames (or on all); results in rank order; the first
        exception is re-raised after all threads have finished."""
        ranks = [r for r in range(self.world) if all_ranks or self.bounds[r][1] > self.bounds[r][0]]
        futs = {r: self._pools[r].submit(fn, r) for r in ranks}
        out, err = [], None
        for r in ranks:
            try:
                out.append(futs[r].result())
            except Exception as e:        # noqa: BLE001 -- collected, re-raised below
                out.append(None)
                err = err or e
        if err is not None:
            raise err
        return out

    def _set_frames(self, n_frames: int):
        if n_frames > self.max_frames:
            raise ValueError("n_frames exceeds max_frames")
        self.n_frames = int(n_frames)
        self.bounds = [shard_bounds(self.n_frames, r, self.world) for r in range(self.world)]

    def _join(self, per_rank: List[List]) -> List:
        out: List = []
        for part in per_rank:
            out.extend(part)
        if len(out) != self.n_frames:
            raise RuntimeError(f"joined {len(out)} per-frame results for {self.n_frames} frames")
        return out

    def owner(self, frame: int) -> Tuple[int, int]:
        """(rank, local frame index) of a global frame index."""
        if not 0 <= frame < self.n_frames:
            raise IndexError(frame)
        r = frame * self.world // self.n_frames
        return r, frame - self.bounds[r][0]

    # ------------------------------------------------------------------ input
    def load(self, cubes: np.ndarray):
        cubes = np.asarray(cubes)
        if cubes.ndim != 4 or tuple(cubes.shape[1:]) != self.shape:
            raise ValueError(f"expected [F, {self.shape[0]}, {self.shape[1]}, {self.shape[2]}] cubes, got {cubes.shape}")
        self._set_frames(cubes.shape[0])
        self._each(lambda r: self.parts[r].load(cubes[self.bounds[r][0]:self.bounds[r][1]]))

    def synth(self, n_frames: int, seed0: int, **kw):
        """Frame f of the batch is generated from seed0 + f whichever device it lands on."""
        self._set_frames(n_frames)
        self._each(lambda r: self.parts[r].synth(self.bounds[r][1] - self.bounds[r][0], seed0 + self.bounds[r][0], **kw))

    def cubes(self) -> np.ndarray:
        V, S, C = self.shape
        out = np.empty((self.n_frames, V, S, C), dtype=np.complex64)

        def fetch(r):
            lo, hi = self.bounds[r]
            out[lo:hi] = self.parts[r].cubes(0, hi - lo)
        self._each(fetch)
        return out

    # ------------------------------------------------------------------ compute
    def detect(self) -> List[np.ndarray]:
        self.dets = self._join(self._each(lambda r: self.parts[r].detect()))
        return self.dets

    def point_clouds(self) -> List[np.ndarray]:
        pcs = self._join(self._each(lambda r: self.parts[r].point_clouds()))
        live = [p for r, p in enumerate(self.parts) if self.bounds[r][1] > self.bounds[r][0]]
        self.dets = self._join([p.dets for p in live])
        self.n_refined = sum(p.n_refined for p in live)
        return pcs

    def integrated_power(self) -> np.ndarray:
        """``FramePipeline.integrated_power`` of every shard (``integrate_rx=`` among the pipeline keywords), joined in frame order:
        float64 ``[F, S, C]``."""
        _, S, C = self.shape
        parts = self._each(lambda r: self.parts[r].integrated_power())
        out = np.concatenate(parts) if parts else np.zeros((0, S, C))
        if len(out) != self.n_frames:
            raise RuntimeError(f"joined {len(out)} power planes for {self.n_frames} frames")
        return out

    def ego_velocities(self, estimator) -> np.ndarray:
        """``FramePipeline.ego_velocities``: every device fits the frames of its shard (``ego_fits``), the estimator's state
        runs once over the joined fits in frame order."""
        live = [r for r in range(self.world) if self.bounds[r][1] > self.bounds[r][0]]
        per_rank = self._each(lambda r: self.parts[r].ego_fits(estimator))
        fits = np.concatenate([f for f, _ in per_rank]) if per_rank else np.empty((0, 4))
        counts = np.concatenate([c for _, c in per_rank]) if per_rank else np.empty(0, dtype=np.int32)
        if len(counts) != self.n_frames:
            raise RuntimeError(f"joined {len(counts)} per-frame fits for {self.n_frames} frames")
        self.n_ego_flagged = sum(getattr(self.parts[r], "n_ego_flagged", 0) for r in live)
        return ego_state_scan(estimator, fits, counts)

    def vehicle_velocities(self, estimator, initial=None, track: bool = False, only_2D: bool = True) -> np.ndarray:
        """``FramePipeline.vehicle_velocities`` for independent frames: every device fits the frames of its shard
        (``vehicle_fits`` with its rows of ``initial``, all from one seed: ``vehicle_seed``), the estimator's state runs once over
        the joined fits in frame order.  ``track=True`` is refused: a chain hands every frame's estimate to the next one, so it
        cannot be split by frames -- use one ``FramePipeline``."""
        import copy
        import os
        if track:
            raise ValueError("MultiDeviceFramePipeline.vehicle_velocities cannot take track=True: the chain runs through the "
                             "frames in order, so it cannot be split across devices -- use one FramePipeline")
        dim = 2 if only_2D else 3
        init = None
        if initial is not None:
            init = np.asarray(initial, dtype=np.float64)
            if init.shape != (self.n_frames, dim):
                raise ValueError(f"vehicle_velocities: initial must have shape {(self.n_frames, dim)}, got {init.shape}")
        est = copy.copy(estimator)
        if est.seed is None:
            est.seed = int.from_bytes(os.urandom(8), "little")
        self.vehicle_seed = est.seed
        live = [r for r in range(self.world) if self.bounds[r][1] > self.bounds[r][0]]
        per_rank = self._each(lambda r: self.parts[r].vehicle_fits(
            est, None, None if init is None else init[self.bounds[r][0]:self.bounds[r][1]], False, only_2D))
        fits = np.concatenate([f for f, _ in per_rank]) if per_rank else np.zeros((0, dim + 2))
        status = np.concatenate([s for _, s in per_rank]) if per_rank else np.zeros(0, dtype=np.int32)
        if len(fits) != self.n_frames:
            raise RuntimeError(f"joined {len(fits)} per-frame fits for {self.n_frames} frames")
        self.n_vehicle_flagged = sum(getattr(self.parts[r], "n_vehicle_flagged", 0) for r in live)
        return vehicle_state_scan(estimator, fits, status)

    def doppler_azimuth_velocities(self, estimator, altitudes, enable_precise_responses=False) -> np.ndarray:
        """``FramePipeline.doppler_azimuth_velocities``: every device fits the frames of its shard (``doppler_azimuth_fits`` with
        its rows of ``altitudes``), the estimator's state runs once over the joined fits in frame order."""
        alt = np.asarray(altitudes, dtype=np.float64)
        if alt.ndim == 0:
            alt = np.full(self.n_frames, float(alt))
        if alt.shape != (self.n_frames,):
            raise ValueError(f"doppler_azimuth_velocities: altitudes must be {self.n_frames} numbers or one, got shape {alt.shape}")
        live = [r for r in range(self.world) if self.bounds[r][1] > self.bounds[r][0]]
        per_rank = self._each(lambda r: self.parts[r].doppler_azimuth_fits(estimator, alt[self.bounds[r][0]:self.bounds[r][1]],
                                                                          enable_precise_responses))
        if not per_rank:
            return np.zeros((0, 3))
        fits = np.concatenate([f for f, _ in per_rank])
        status = np.concatenate([s for _, s in per_rank])
        if len(fits) != self.n_frames:
            raise RuntimeError(f"joined {len(fits)} per-frame fits for {self.n_frames} frames")
        self.n_dopaz_fits_flagged = sum(getattr(self.parts[r], "n_dopaz_fits_flagged", 0) for r in live)
        return dopaz_state_scan(estimator, fits, status)

    def micro_doppler(self, target_ranges=(0, 1.0), rx_idx: int = 0) -> np.ndarray:
        """``FramePipeline.micro_doppler`` of every shard, concatenated in frame order (the rows are independent of each other;
        ``micro_doppler_history`` of the result is the spectrogram)."""
        rows = self._join(self._each(lambda r: self.parts[r].micro_doppler(target_ranges, rx_idx)))
        return np.asarray(rows, dtype=np.float64).reshape(self.n_frames, self.shape[2])

    def strip_map_sar(self, proc, velocities, sensor_height_m: float = 0.24, rx_index: int = 0, max_SAR_distance: float = 1.5):
        """``FramePipeline.strip_map_sar`` of every shard on its rows of ``velocities``, joined in frame order (a frame's slice
        depends on that frame alone): ``(slices, windows)``."""
        vel = np.asarray(velocities, dtype=np.float64)
        if vel.ndim == 0:
            vel = np.full(self.n_frames, float(vel))
        if vel.shape != (self.n_frames,):
            raise ValueError(f"strip_map_sar: velocities must be {self.n_frames} numbers or one, got shape {vel.shape}")
        per_rank = self._each(lambda r: self.parts[r].strip_map_sar(proc, vel[self.bounds[r][0]:self.bounds[r][1]], sensor_height_m,
                                                                   rx_index, max_SAR_distance))
        slices = self._join([p[0] for p in per_rank])
        wins = [np.asarray(p[1], dtype=np.int32).reshape(-1, 4) for p in per_rank]
        return slices, (np.concatenate(wins) if wins else np.zeros((0, 4), dtype=np.int32))

    def range_detections(self, detector, chirp_idx: int = 0, return_thresholds: bool = False):
        """``FramePipeline.range_detections`` of every shard, joined in frame order (the detector keeps no state across frames)."""
        per_rank = self._each(lambda r: self.parts[r].range_detections(detector, chirp_idx, return_thresholds))
        if not return_thresholds:               # no shard writes or downloads a threshold table nobody asked for
            return self._join(per_rank)
        dets = self._join([p[0] for p in per_rank])
        thr = [np.asarray(p[1], dtype=np.float64).reshape(-1, self.shape[1]) for p in per_rank]
        return dets, (np.concatenate(thr) if thr else np.zeros((0, self.shape[1])))

    def capon_range_angle(self, thetas_rad, rx_antennas, range_bins=None, delta: float = 1e-3, perform_windowing: bool = True,
                          frames_per_pass: Optional[int] = None) -> np.ndarray:
        """``FramePipeline.capon_range_angle`` of every shard on its own frames, concatenated in frame order (a frame's map does
        not depend on the other frames)."""
        th, _, (r_lo, r_hi), _, _ = capon_cube_args(self.shape[0], self.shape[1], thetas_rad, rx_antennas, range_bins, delta,
                                                    frames_per_pass)
        per_rank = self._each(lambda r: self.parts[r].capon_range_angle(thetas_rad, rx_antennas, range_bins, delta,
                                                                        perform_windowing, frames_per_pass))
        maps = self._join([np.asarray(p, dtype=np.float64) for p in per_rank])
        return np.asarray(maps, dtype=np.float64).reshape(self.n_frames, r_hi - r_lo, len(th))

    def capon_point_clouds(self, thetas_rad, rx_antennas, detector, range_bins=None, delta: float = 1e-3,
                           perform_windowing: bool = True, doppler_windowing: bool = True,
                           frames_per_pass: Optional[int] = None) -> List[np.ndarray]:
        """``FramePipeline.capon_point_clouds`` of every shard on its own frames, joined in frame order (a frame's point cloud
        does not depend on the other frames); ``capon_dets``, ``capon_doppler_idx`` and ``capon_peak`` are joined likewise."""
        capon_points_args(self.shape[0], self.shape[1], self.shape[2], thetas_rad, rx_antennas, detector, range_bins, delta,
                          frames_per_pass)
        pcs = self._join(self._each(lambda r: self.parts[r].capon_point_clouds(
            thetas_rad, rx_antennas, detector, range_bins, delta, perform_windowing, doppler_windowing, frames_per_pass)))
        live = [p for r, p in enumerate(self.parts) if self.bounds[r][1] > self.bounds[r][0]]
        self.capon_dets = self._join([p.capon_dets for p in live])
        self.capon_doppler_idx = self._join([p.capon_doppler_idx for p in live])
        self.capon_peak = self._join([p.capon_peak for p in live])
        return pcs

    def doppler_azimuth(self, proc, rx_sets, range_windows, shift_angle=True, precise_vel_ranges=None):
        """``FramePipeline.doppler_azimuth`` of every shard on its rows of the per-frame tables, joined in frame order (the frames
        are independent of each other)."""
        rw = _per_frame_pairs("range_windows", range_windows, self.n_frames)
        pv = None if precise_vel_ranges is None else _per_frame_pairs("precise_vel_ranges", precise_vel_ranges, self.n_frames)

        def run(r):
            lo, hi = self.bounds[r]
            return self.parts[r].doppler_azimuth(proc, rx_sets, rw[lo:hi], shift_angle, None if pv is None else pv[lo:hi])
        per_rank = self._each(run)
        if pv is None:
            if not per_rank:
                raise ValueError("doppler_azimuth: no frames are resident")
            return np.concatenate(per_rank, axis=1)
        maps, bins = [], []
        for part_maps, part_bins in per_rank:
            n = len(part_bins)
            maps.extend(part_maps[:, f] if isinstance(part_maps, np.ndarray) else part_maps[f] for f in range(n))
            bins.extend(part_bins)
        if len(bins) != self.n_frames:
            raise RuntimeError(f"joined {len(bins)} per-frame maps for {self.n_frames} frames")
        if maps and all(x.shape == maps[0].shape for x in maps):
            return np.stack(maps, axis=1), bins
        return maps, bins

    def doppler_azimuth_peaks(self, proc, rx_sets, groups, range_windows, shift_angle=True, precise_vel_ranges=None,
                              min_threshold_dB=30.0):
        """``FramePipeline.doppler_azimuth_peaks`` of every shard on its rows of the per-frame tables; the per-frame lists of every
        group joined in frame order.  ``n_peaks_undecided`` is the sum over the shards."""
        rw = _per_frame_pairs("range_windows", range_windows, self.n_frames)
        pv = None if precise_vel_ranges is None else _per_frame_pairs("precise_vel_ranges", precise_vel_ranges, self.n_frames)

        def run(r):
            lo, hi = self.bounds[r]
            part = self.parts[r]
            res = part.doppler_azimuth_peaks(proc, rx_sets, groups, rw[lo:hi], shift_angle, None if pv is None else pv[lo:hi],
                                             min_threshold_dB)
            return res, part.n_peaks_undecided
        per_rank = self._each(run)
        if not per_rank:
            raise ValueError("doppler_azimuth_peaks: no frames are resident")
        G = len(per_rank[0][0][0])
        row_peaks = [self._join([res[0][g] for res, _ in per_rank]) for g in range(G)]
        zero_az = [self._join([res[1][g] for res, _ in per_rank]) for g in range(G)]
        self.n_peaks_undecided = sum(n for _, n in per_rank)
        return row_peaks, zero_az

    def chain3d(self, magnitude: bool = False, out: Optional[np.ndarray] = None) -> Optional[np.ndarray]:
        """3-D windowed FFT of every frame on its device.  ``out`` (optional, caller-owned ``[F, A, S, C]`` complex64 /
        float32 array): every device thread copies its frames into its own slice of it."""
        self._each(lambda r: self.parts[r].chain3d(magnitude))
        if out is None:
            return None
        if out.shape[0] < self.n_frames:
            raise ValueError("output array holds fewer frames than the batch")

        def fetch(r):
            lo, hi = self.bounds[r]
            for f in range(lo, hi):
                out[f] = self.parts[r].fetch_chain3d(f - lo)
        self._each(fetch)
        return out

    def fetch_chain3d(self, frame: int) -> np.ndarray:
        r, local = self.owner(frame)
        return self._pools[r].submit(self.parts[r].fetch_chain3d, local).result()

    def close(self):
        for r, pool in enumerate(self._pools):
            part = self.parts[r]

            def shut(p=part):
                if hasattr(p, "bufs"):
                    p.bufs.free()
                ctx = getattr(p, "ctx", None)
                if ctx is not None and ctx is not _lib._default_ctx:
                    ctx.close()
            try:
                pool.submit(shut).result()
            finally:
                pool.shutdown(wait=True)
        self.parts = []
