"""Inputs and error bounds for the Capon / MVDR tests (test_capon_cases_host.py, test_gpu_capon.py).  Pure NumPy.

Every builder yields `(name, X, thetas, delta, tol_terms)`: X complex64 [F][V][R][K] as mmw_capon takes it, the angle
grid in radians, the diagonal loading, and a dict of what the assertions need (`cond2` [F][R]: the 2-norm condition
number of each bin's loaded covariance, computed in float64 from the complex128 matrix; other keys per family).

Four families:
  second_pass_shapes(num_cu)  bin counts above the grid cap of k_capon_sweep, so that waves take a second (third) bin:
                              the division-free (frame, bin) advance, the `more` branch, the hand-over of the two
                              prefetch slots to the next bin for one, two and three snapshot chunks
  edge_shapes()               single-trip, tiny: every register-row count, chunk count and chunk tail
  conditioned_cases()         cond2 of the loaded covariance from ~1e1 to ~1e10, and bins scaled by ~1e-20 / ~1e+15
  poison_cases(num_cu)        multi-trip batches with a NaN in one bin and an Inf in another
"""
import numpy as np

# The float64 NumPy oracle (oracle_np.capon_spectrum: X X^H / K, np.linalg.solve, 1 / Re(a^H R^-1 a)) against a 50-digit
# mpmath evaluation of the same definition on conditioned_cases(): err / (cond2 * 2**-53) per bin was 0.08 .. 0.37 on
# the 25 bins with cond2 from 4.6e3 to 5.2e9 and 0.38 / 0.79 / 0.89 on the three scaled bins with cond2 = 5.3, where the
# error is four ulps of float64 whatever the conditioning (test_capon_cases_host.py prints the table).  C_ORACLE is twice
# the largest ratio, 0.89, rounded up to one significant digit; the factor two covers the spread between seeds.
C_ORACLE = 2.0
# The device's share of the bound.  V = 16 sweeps, each adding rounding errors of order u * cond2 to the quadratic form.
# Observed on an MI355X (256 CUs) over conditioned_cases() and edge_shapes(), err = max |P - oracle| / oracle per case:
#   cond2 4.4e9 .. 5.2e9 (K < V, delta 1e-9)   err 2.2e-7   err / (cond2 2^-53) = 0.26 .. 0.42
#   cond2 2.6e7 .. 3.5e7 (60 dB, delta 0)      err 5.4e-8   (float32 rounding alone: 2^-24 = 6.0e-8)
#   cond2 7.0e6 .. 9.0e6 (K < V, delta 1e-6)   err 5.3e-8   (the same)
#   every other case, cond2 1 .. 4e5           err 0.9e-8 .. 5.9e-8, all below 2^-24
# Only the first row has an error above the float32 rounding of the output, so only there does the ratio say anything
# about the sweep: 0.42, the oracle's own 0.17 .. 0.29 on those bins included.  That is below V / 4 = 4, so C_KERNEL
# stays at V = 16 ("Capon numerics", has the table).
C_KERNEL = 16.0
OBSERVED_KERNEL_RATIO = 0.42

T_VALUES = (1, 63, 64, 192, 193, 200)                       # 192 = angles held in the LDS table; 64 = one per lane
VK_VALUES = ((2, 4), (5, 32), (12, 40), (16, 96), (9, 65))   # one chunk x2; two chunks + tail; three aligned; three + tail
EDGE_V = (1, 2, 4, 5, 8, 9, 12, 13, 16)
EDGE_K = (1, 2, 31, 32, 33, 63, 64, 65, 97)
EDGE_R = (1, 3, 5)


def grid_cap_bins(num_cu):
    """Bins one launch of k_capon_sweep covers in its first trip: capon() in csrc/mmw_beamform.h launches
    min(ceil(bins / 4), 4 * num_cu) workgroups of four waves, one bin per wave and trip, so a wave takes a second bin
    exactly when n_frames * R exceeds 16 * num_cu."""
    return 16 * num_cu


def bound(cond2):
    """Relative error allowed between the float32 device spectrum and the float64 oracle: one float32 rounding of the
    output plus one for the final reciprocal's conversion, and the kernel's and the oracle's own share of cond2 * u."""
    return 2.0 ** -23 + (C_KERNEL + C_ORACLE) * np.asarray(cond2, dtype=np.float64) * 2.0 ** -53


def loaded_covariance(X, delta):
    """[F][V][R][K] complex64 -> [F][R][V][V] complex128: X X^H / K + delta tr / V I, inputs promoted exactly."""
    Xb = np.ascontiguousarray(np.swapaxes(X, 1, 2)).astype(np.complex128)       # [F][R][V][K]
    V, K = Xb.shape[2], Xb.shape[3]
    Rm = Xb @ np.conj(np.swapaxes(Xb, 2, 3)) / K
    tr = np.real(np.trace(Rm, axis1=2, axis2=3))
    return Rm + (delta * tr / V)[..., None, None] * np.eye(V)


def cond2(X, delta):
    """2-norm condition number of every bin's loaded covariance, [F][R] float64."""
    s = np.linalg.svd(loaded_covariance(X, delta), compute_uv=False)
    return s[..., 0] / s[..., -1]


def steering(V, theta):
    return np.exp(-1j * np.pi * np.arange(V) * np.sin(theta))


def _noise(rng, shape):
    return rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)


def _thetas(T, seed):
    if T == 1:
        return np.array([0.3])
    th = np.linspace(-1.35, 1.35, T)
    return th + np.random.default_rng(seed).uniform(-1e-3, 1e-3, T)        # no symmetric grid: +theta and -theta differ


def _batch(seed, F, V, R, K, src_amp=4.0):
    """Noise plus one source per bin at an angle that depends on the bin: a bin computed from another bin's snapshots
    (a wrong advance, a prefetch slot handed to the wrong bin) differs by far more than any tolerance."""
    rng = np.random.default_rng(seed)
    X = _noise(rng, (F, V, R, K))
    th0 = rng.uniform(-1.2, 1.2, (F, 1, R, 1))
    a = np.exp(-1j * np.pi * np.arange(V).reshape(1, V, 1, 1) * np.sin(th0))
    X += (src_amp * a * _noise(rng, (F, 1, R, K))).astype(np.complex64)
    return X.astype(np.complex64)


# ----------------------------------------------------------------------------------------------------- second pass
def second_pass_table(num_cu):
    """(name, F, R, V, K, T) of every second-pass case.  Five shapes F x R whose bin count crosses the cap c in each way
    the advance bin -> bin + c can go wrong, each with two of the five (V, K); every T of T_VALUES occurs."""
    c = grid_cap_bins(num_cu)
    shapes = (("one_wave_second_bin", 1, c + 1),              # step_f = 1, step_r = c - R ... : one wave takes a second bin
              ("wrap_into_frame_1", 2, c + 3),                # step_f = 0: nr + step_r wraps into frame 1
              ("step_f_1", 3, c // 2 + 7),                    # step_f = 1, step_r != 0
              ("r1_three_trips", 2 * c + 5, 1),               # R = 1: step_r = 0, step_f = c, three trips
              ("step_f_large", c // 3 + 2, 7))                # step_f = c // 7
    # the largest (V, K) go with the smallest bin counts (a case stays below 80 MB)
    pairs = ((0, 3), (0, 2), (1, 0), (1, 4), (2, 1), (2, 3), (3, 1), (3, 4), (4, 0), (4, 2))
    ts = (200, 63, 1, 193, 64, 192, 200, 63, 193, 64)
    out = []
    for (si, vi), T in zip(pairs, ts):
        name, F, R = shapes[si]
        V, K = VK_VALUES[vi]
        out.append((f"{name}_V{V}_K{K}_T{T}", F, R, V, K, T))
    return out


def second_pass_case(num_cu, name):
    for i, (nm, F, R, V, K, T) in enumerate(second_pass_table(num_cu)):
        if nm == name:
            X = _batch(4100 + i, F, V, R, K)
            return nm, X, _thetas(T, i), 1e-2, {"three_trips": nm.startswith("r1_three_trips")}
    raise KeyError(name)


def second_pass_shapes(num_cu):
    for row in second_pass_table(num_cu):
        yield second_pass_case(num_cu, row[0])


# ------------------------------------------------------------------------------------------------------------ edges
def edge_shapes():
    """Single trip, F = 2: every V (register rows per lane 1..4, with and without padding lanes), every K (chunks of 32:
    one snapshot, a pair, one short of / exactly / one past one and two chunks, four chunks), every R."""
    table = ((1, 1, 1, 7), (2, 2, 3, 64), (4, 31, 5, 63), (5, 32, 1, 200), (8, 33, 3, 7), (9, 63, 5, 193),
             (12, 64, 1, 65), (13, 65, 3, 192), (16, 97, 5, 200), (16, 1, 3, 7), (1, 97, 5, 1), (13, 32, 1, 64))
    for i, (V, K, R, T) in enumerate(table):
        X = _batch(5200 + i, 2, V, R, K, src_amp=2.0)
        delta = 1e-2
        yield f"edge_V{V}_K{K}_R{R}_T{T}", X, _thetas(T, 50 + i), delta, {"cond2": cond2(X, delta)}


# ------------------------------------------------------------------------------------------------------ conditioning
def _round_bits(x, bits):
    """x rounded to `bits` significant bits."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)


SCALE_SMALL = float(_round_bits(1e-20, 12))      # 1e-20 and 1e+15 to 12 significant bits: times the 11-bit samples of the
SCALE_LARGE = float(_round_bits(1e+15, 12))      # "scaled_bins" case the products are exact in complex64


def conditioned_cases():
    """cond2 of the loaded covariance from ~1e1 to ~1e10 (delta = 0 with K < V is not a case: singular by definition)."""
    th = np.array([-1.2, -0.7, -0.31, -0.05, 0.0, 0.2, 0.55, 0.9, 1.3])

    def done(name, X, delta, **extra):
        X = X.astype(np.complex64)
        return name, X, th, delta, dict(cond2=cond2(X, delta), **extra)

    # K < V: rank-deficient sample covariance, conditioned by the loading alone (cond2 ~ V / delta)
    for i, (V, K, delta) in enumerate(((12, 5, 1e-3), (16, 3, 1e-6), (12, 5, 1e-9))):
        rng = np.random.default_rng(6100 + i)
        yield done(f"rank_deficient_V{V}_K{K}_delta{delta:g}", _noise(rng, (1, V, 4, K)), delta)
    # no loading, K >= 4 V, one source 40 / 60 dB above the noise, at a grid angle (th[6]) in bins 0, 1 and off it in 2, 3
    for i, (V, K, db) in enumerate(((8, 32, 40), (12, 64, 60))):
        rng = np.random.default_rng(6200 + i)
        X = _noise(rng, (1, V, 4, K)) * np.float32(np.sqrt(0.5))
        for r, t0 in enumerate((th[6], th[6], 0.41, -0.93)):
            X[0, :, r, :] += (10.0 ** (db / 20) * steering(V, t0)[:, None] * _noise(rng, (1, K)) * np.sqrt(0.5)).astype(np.complex64)
        yield done(f"one_source_{db}dB_delta0_V{V}_K{K}", X, 0.0)
    # two coherent sources (one waveform): the signal part of the covariance has rank one
    rng = np.random.default_rng(6300)
    V, K = 10, 40
    X = _noise(rng, (1, V, 3, K)) * np.float32(0.05)
    s = _noise(rng, (1, 1, 3, K))
    X += ((steering(V, th[2]) + 0.8j * steering(V, th[7])).reshape(1, V, 1, 1) * s * 30.0).astype(np.complex64)
    yield done("two_coherent_sources_delta1e-4", X, 1e-4)
    # two uncorrelated sources, all sixteen antennas
    rng = np.random.default_rng(6400)
    V, K = 16, 64
    X = _noise(rng, (1, V, 2, K))
    for t0, amp in ((th[1], 20.0), (0.1, 5.0)):
        X += (amp * steering(V, t0).reshape(1, V, 1, 1) * _noise(rng, (1, 1, 2, K))).astype(np.complex64)
    yield done("two_sources_delta1e-4_V16", X, 1e-4)
    # one well-conditioned bin, then the same bin times ~1e-20 and times ~1e+15.  P scales with the power, so the loaded
    # matrix stays equally conditioned and P(s X) = s^2 P(X).  The samples are multiples of 4 below 2^13 (11 significant
    # bits) and the scales have 12, so s X is exact in complex64 and the property is a statement about the kernel alone;
    # the amplitude keeps s^2 P inside the NORMAL float32 range (1.2e-38 .. 3.4e38) the output has.
    rng = np.random.default_rng(6500)
    V, K = 8, 32
    X0 = (rng.integers(-2047, 2048, (1, V, 1, K)) * 4.0 + 4j * rng.integers(-2047, 2048, (1, V, 1, K)))
    X = np.concatenate((X0, X0 * SCALE_SMALL, X0 * SCALE_LARGE), axis=2)
    assert np.array_equal(X.astype(np.complex64).astype(np.complex128), X)
    yield done("scaled_bins", X, 1e-2, scales=(1.0, SCALE_SMALL, SCALE_LARGE))


# ----------------------------------------------------------------------------------------------------------- poison
def poison_cases(num_cu):
    """Multi-trip batches; tol_terms["poison"] lists (frame, antenna, bin, snapshot, value, original): X holds `value`
    there, the clean batch `original`.  A NaN and an Inf, in antenna 0 (which the padding lanes li >= V read again) and
    in the last antenna, in the last snapshot (the tail chunk), in bins of the first and of a later trip."""
    c = grid_cap_bins(num_cu)
    table = second_pass_table(num_cu)
    picks = ((next(n for n in table if n[0].startswith("step_f_1") and n[3] == 5)[0], 0),
             (next(n for n in table if n[0].startswith("one_wave_second_bin") and n[3] == 12)[0], -1),
             (next(n for n in table if n[0].startswith("wrap_into_frame_1") and n[3] == 9)[0], 0))
    for name, ant in picks:
        _, X, th, delta, _ = second_pass_case(num_cu, name)
        F, V, R, K = X.shape
        ant %= V
        n_bins = F * R
        # a NaN in a first-trip bin whose wave goes on to a second one (with n_bins = c + 1 that is bin 0 alone: its wave
        # has bin c in flight while it works on the NaN); an Inf in the last bin of all (a later trip); with several frames
        # also a NaN in a second-trip bin
        assert n_bins - c > 3 or F == 1
        bins = [(0 if n_bins - c <= 3 else 3, np.nan), (n_bins - 1, np.inf)]
        if F > 1:
            bins.append((c + 2, np.nan))
        poison = []
        for b, val in bins:
            f, r = divmod(b, R)
            k = K - 1
            poison.append((f, ant, r, k, val, complex(X[f, ant, r, k])))
            X[f, ant, r, k] = complex(val, 1.0) if np.isinf(val) else complex(1.0, val)
        yield f"poison_ant{ant}_{name}", X, th, delta, {"poison": poison}
