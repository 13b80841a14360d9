"""The float64 NumPy restatement of antenna-integrated (non-coherent) CFAR detection and the seeded cases of its
tests (test_integrated_cases_host.py, test_gpu_integrated_detect.py).  Pure NumPy + the oracle; nothing here touches a device.

Restatement, per frame and antenna list `ants` (order as given):
    RD_v   = oracle_np.range_doppler(cube)[v]                 complex128: fftshift_C(fft2(hann(S) hann(C) cube[v]))
    P[r,d] = sum_{v in ants, list order} re(RD_v)^2 + im(RD_v)^2
    dets   = oracle_np.ca_cfar_2d / os_cfar_2d (used as they are, strict >) on P
The angle estimates of the detections are oracle_np.angle_argmax's, unchanged.  No upstream implementation exists.

Cases: the smallest shapes that reach each route of mmw_range_doppler_power64 (the persistent 256 x 128 kernel, the same shape
below its batch threshold, an LDS-resident single-pass plane, a small power-of-two plane and a plane beyond the LDS, both
two-pass), each with the full list, [0] and a permuted subset, under CA and (where the window fits the plane) OS CFAR.

Margin: detections can be demanded identical only where no valid cell sits at its threshold to within the float64 error of P.
margin() returns the smallest |P - T| / T over the valid cells; the host test asserts it is >= MARGIN for every case (a
condition on the seeds, not a tolerance), so the GPU test skips no frame.
"""
import functools
from collections import namedtuple

import numpy as np

from mmwave_radar_processing_amd import synth
from oracle import oracle_np as O

import axis_fft_cases as ax

MARGIN = 1e-9
CA = ("ca", (4, 4), (2, 2), 1e-5)               # CaCFAR2D((4, 4), (2, 2), 1e-5)
OS = ("os", (5, 5), (3, 2), 0.7, 2.0)           # the GUI's OsCFAR2D((5, 5), (3, 2), rho=0.7, alpha=2.0)
AZ, EL = list(range(8)), [8, 9, 10, 11]

Case = namedtuple("Case", "name shape seeds ants cfar route")


def _lists(V):
    return {"all": list(range(V)), "one": [0], "perm": [7, 2, 9] if V >= 10 else [3, 0, 2]}


def _cases():
    out = []
    for tag, shape, seeds, route, cfars in (
            ("256x128_f9", (12, 256, 128), tuple(range(4100, 4109)), "persistent", (CA, OS)),
            ("256x128_f3", (12, 256, 128), tuple(range(4100, 4103)), "per_antenna_fused_shape", (CA,)),
            ("63x70", (12, 63, 70), (4201, 4202), "per_antenna_lds", (CA, OS)),
            ("64x64", (12, 64, 64), (4301, 4302), "per_antenna_two_pass", (CA, OS)),
            ("512x64", (4, 512, 64), (4401, 4402), "per_antenna_two_pass", (CA,))):
        for lname, ants in _lists(shape[0]).items():
            for cfar in cfars:
                if tag == "256x128_f9" and cfar is OS and lname != "all":
                    continue            # (one OS run of the large batch: the CFAR kernels are not what the lists vary)
                out.append(Case(f"{tag}-{lname}-{cfar[0]}", shape, seeds, tuple(ants), cfar, route))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def cubes(shape, seeds):
    """[F, V, S, C] complex64, frame i = synth.synth_cube(seeds[i], shape); read-only."""
    x = np.stack([synth.synth_cube(s, shape) for s in seeds])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def rd_planes(shape, seeds):
    """oracle_np.range_doppler of every frame: complex128 [F, V, S, C]; read-only."""
    rd = np.stack([O.range_doppler(c) for c in cubes(shape, seeds)])
    rd.setflags(write=False)
    return rd


def power(rd, ants):
    """P [.., S, C] float64 of rd [.., V, S, C]: re^2 + im^2 of the listed antennas, added in list order."""
    p = None
    for v in ants:
        t = rd[..., v, :, :].real ** 2 + rd[..., v, :, :].imag ** 2
        p = t if p is None else p + t
    return p


def cfar(P, spec):
    """(thr, dets int64 (N, 2)) of one plane under CA / OS."""
    if spec[0] == "ca":
        thr, _, dets = O.ca_cfar_2d(P, spec[1], spec[2], spec[3])
    else:
        thr, _, dets = O.os_cfar_2d(P, spec[1], spec[2], spec[3], spec[4])
    return thr, (np.array(dets, dtype=np.int64) if dets else np.empty((0, 2), dtype=np.int64))


def margin(P, thr):
    """Smallest |P - T| / T over the valid cells (finite T > 0)."""
    ok = np.isfinite(thr) & (thr > 0)
    return float(np.min(np.abs(P[ok] - thr[ok]) / thr[ok])) if ok.any() else np.inf


Reference = namedtuple("Reference", "power thr dets margin")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement of a case: power [F, S, C], per-frame thresholds and detections, the smallest margin."""
    c = BY_NAME[name]
    P = power(rd_planes(c.shape, c.seeds), c.ants)
    res = [cfar(P[f], c.cfar) for f in range(len(c.seeds))]
    P.setflags(write=False)
    return Reference(P, [r[0] for r in res], [r[1] for r in res], min(margin(P[f], r[0]) for f, r in enumerate(res)))


def make_cfar(spec):
    """The package's detector object of a CFAR spec."""
    from mmwave_radar_processing_amd.detectors import CaCFAR2D, OsCFAR2D
    if spec[0] == "ca":
        return CaCFAR2D(spec[1], spec[2], spec[3])
    return OsCFAR2D(spec[1], spec[2], rho=spec[3], alpha=spec[4])


def config(shape):
    """(ConfigManager, oracle scalars) of a cfg with this plane shape."""
    from mmwave_radar_processing_amd.config_managers import ConfigManager
    V, S, C = shape
    txt = synth.synth_cfg_text(num_samples=S, num_loops=C, num_tx=3 if V == 12 else 1)
    cm = ConfigManager()
    cm.load_cfg_text(txt)
    return cm, O.cfg_scalars(txt)


def point_cloud(rd, dets, sc, az=AZ, el=EL, A=64):
    """One frame's (points (N, 4), az_idx, el_idx) from the restatement's detections: oracle_np.point_cloud's tail."""
    if dets.shape[0] == 0:
        return np.empty((0, 4)), np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64)
    rbins, vbins = O.rd_bins(sc)
    _, abins = O.angle_tables(A)
    r, v = dets[:, 0], dets[:, 1]
    az_i, _ = O.angle_argmax(rd, r, v, az, A, True)
    el_i, _ = O.angle_argmax(rd, r, v, el, A, False)
    a, e = abins[az_i], abins[el_i]
    rng = rbins[r]
    return np.column_stack((rng * np.cos(e) * np.cos(a), rng * np.cos(e) * np.sin(a), rng * np.sin(e), vbins[v])), az_i, el_i


def power_bound(cube, rd, ants):
    """The bound of the issue on |P_device - P| for one frame, from the project's own figure for one antenna's float64 |RD| plane
    (axis_fft_cases.mag64_ulps against the plane's L1 norm):  delta_v = mag64_ulps(S, C) 2^-53 l1_v,
        |dP| <= sum_v (2 |RD_v| + delta_v) delta_v + (n_ants + 2) 2^-53 P."""
    V, S, C = cube.shape
    w = np.hanning(S)[:, None] * np.hanning(C)[None, :]
    bound = np.zeros((S, C))
    for v in ants:
        l1 = float(ax.abs1(cube[v].astype(np.complex128) * w).sum())
        delta = ax.mag64_ulps(S, C) * ax.EPS64 * l1
        bound += (2.0 * np.abs(rd[v]) + delta) * delta
    return bound + (len(ants) + 2) * ax.EPS64 * power(rd, ants)


# ------------------------------------------------------------------ the weak-target cube
WEAK_SHAPE, WEAK_SEED, WEAK_CELL, WEAK_AMP = (12, 64, 64), 4504, (20, 43), 3.75


@functools.lru_cache(maxsize=None)
def weak_cube():
    """Noise of synth.synth_cube (no targets, sigma 30) plus one on-bin tone, the same in every antenna.  Its cell is 1.26 times
    the CA threshold on the 12-antenna power plane, 0.83 times on antenna 0's power plane (whose noise sample happens to cancel
    part of the tone: the sum over 12 antennas averages such samples out) and far below the threshold on antenna 0's |RD| plane,
    the one the reference thresholds (the same alpha applied to a magnitude asks for ~ 11 noise rms, to a power for ~ 3.5)."""
    V, S, C = WEAK_SHAPE
    r, d = WEAK_CELL
    noise = synth.synth_cube(WEAK_SEED, WEAK_SHAPE, num_targets=0)
    n, m = np.arange(S)[:, None], np.arange(C)[None, :]
    tone = WEAK_AMP * np.exp(2j * np.pi * (r * n / S + (d - C // 2) * m / C))
    x = noise.astype(np.complex128) + tone[None]
    x = (np.rint(x.real) + 1j * np.rint(x.imag)).astype(np.complex64)
    x.setflags(write=False)
    return x
