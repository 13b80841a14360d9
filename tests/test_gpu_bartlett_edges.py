"""mmw_bartlett straight through the C ABI on crafted geometry, operands and shapes, through every kernel path.

Inputs and exact references: tests/bartlett_cases.py (tests/test_bartlett_cases_host.py asserts, without a GPU, that a kernel
which reduced the phase in float32 would miss the bar at the large spans, that the scaled operands stay normal and that the
impulse list holds both sides of every K-split boundary).

| test                         | what is crafted                                                                              |
|------------------------------|----------------------------------------------------------------------------------------------|
| exact phases                 | dyadic geometry of +-0.05 / 4 / 16 m with turns of exactly 0, +-n, n + 1/2 and beyond 2^11     |
| power-of-two scaling         | 2^k X against 2^k Y as bit patterns, k = -30, -8, 13, 27; an all-ones-mantissa operand         |
| impulses                     | one-hot X per frame: every k at a chunk, group, half-row and K-split boundary, every row tile  |
| batch independence           | frame f of a 5-frame call against a 1-frame call, as bit patterns                              |
| containment                  | a NaN / +inf frame of X, a NaN frame of P, one element of 3e38                                 |
| the entry                    | every refused argument, n_frames = 0, S = 1, S = 2, E = 1, T = 1, T = 5                        |

The bar is SPEC_TOL = 1e-5 of the peak magnitude of that frame's float64 reference, frame by frame.  The output buffer is
poisoned before every call and has guard elements behind it.  Measured worst ratios are printed per path.
"""
import contextlib

import numpy as np
import pytest

import bartlett_cases as bc
from mmwave_radar_processing_amd import _lib
from test_gpu_synth_array import PATHS

pytestmark = pytest.mark.gpu

SPEC_TOL = bc.SPEC_TOL
POISON = np.frombuffer(np.array([0x7FC00ABC, 0x7FC00DEF], dtype=np.uint32).tobytes(), dtype=np.complex64)[0]
POISON_BITS = np.array([POISON]).view(np.uint64)[0]
GUARD = 64
TILE_PATHS = ("tile32 f32", "tile32 bf16x3", "tile32 poly", "tile16")      # the tile size is forced: one kernel whatever the batch
GEMM_PATHS = ("gemm bf16x3", "gemm f32")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.complex64).view(np.uint64)


@contextlib.contextmanager
def forced(ctx, name):
    try:
        for key, val in PATHS[name].items():
            ctx.set_option(key, val)
        yield
    finally:
        for key in PATHS[name]:
            ctx.set_option(key, None)


class Device:
    """Operand buffers for up to F frames of one shape and a poisoned [F][S][T] output with guard elements behind it."""

    def __init__(self, F, S, E, T):
        self.ctx = _lib.default_context()
        self.F, self.S, self.E, self.T = F, S, E, T
        self.cap = F * S * T + GUARD
        self.d_X, self.d_P = self.ctx.alloc(F * S * E * 8), self.ctx.alloc(F * 3 * E * 8)
        self.d_dirs, self.d_out = self.ctx.alloc(3 * T * 8), self.ctx.alloc(self.cap * 8)

    def poison(self):
        self.d_out.upload(np.full(self.cap, POISON, dtype=np.complex64))

    def raw(self):
        self.ctx.sync()
        return self.d_out.download((self.cap,), np.complex64)

    def untouched(self):
        return bool(np.all(bits(self.raw()) == POISON_BITS))

    def load(self, X, P, dirs):
        assert X.dtype == np.complex64 and X.shape[1:] == (self.S, self.E) and len(X) <= self.F and P.shape == (len(X), 3, self.E)
        self.d_X.upload(X)
        self.d_P.upload(np.ascontiguousarray(P, dtype=np.float64))
        self.d_dirs.upload(np.ascontiguousarray(dirs, dtype=np.float64).reshape(3, self.T))

    def call(self, n, lam_m, **over):
        a = dict(ctx=self.ctx.handle, X=self.d_X.ptr, P=self.d_P.ptr, dirs=self.d_dirs.ptr, out=self.d_out.ptr, n_frames=n,
                 S=self.S, E=self.E, T=self.T, lam=lam_m)
        a.update(over)
        return self.ctx.lib.mmw_bartlett(a["ctx"], a["X"], a["P"], a["dirs"], a["out"], a["n_frames"], a["S"], a["E"], a["T"], a["lam"])

    def run(self, X, P, dirs, lam):
        """Poison, upload, call; the guard and everything behind the n frames untouched, every output written; [n, S, T]."""
        self.poison()
        self.load(X, P, dirs)
        _lib.check(self.call(len(X), lam))
        raw, n = self.raw(), len(X) * self.S * self.T
        assert np.all(bits(raw[n:]) == POISON_BITS), "written behind the output"
        assert not np.any(bits(raw[:n]) == POISON_BITS), "an output element was not written"
        return raw[:n].reshape(len(X), self.S, self.T).copy()

    def run_case(self, c, frames=slice(None)):
        return self.run(c["X"][frames], c["P"][frames], c["dirs"], c["lam"])

    def free(self):
        for b in (self.d_X, self.d_P, self.d_dirs, self.d_out):
            b.free()


@contextlib.contextmanager
def device(F, shape):
    dev = Device(F, *shape)
    try:
        yield dev
    finally:
        dev.free()


def report(title, worst):
    print(f"{title}: " + ", ".join(f"{p} {w:.2e}" for p, w in worst.items()))
    assert max(worst.values()) <= SPEC_TOL, worst


# ------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("span", list(bc.SPANS) + ["unit vectors"])
@pytest.mark.parametrize("shape", ["masked", "fast"])
def test_exact_phases_on_every_path(shape, span):
    """Turns of exactly 0, +-n and n + 1/2 and, at +-4 m and +-16 m, beyond 2^11 with the 2^-14 bit set: a phase reduced in
    anything narrower than float64 misses the bar by 4 x and more here (host test).  `unit vectors`: steering_dirs at 77 GHz on
    positions uniform in +-4 m, against oracle.bartlett_response."""
    dims = bc.MASKED if shape == "masked" else bc.FAST
    c = bc.unit_case(dims) if span == "unit vectors" else bc.dyadic_case(dims, span)
    with device(2, dims) as dev:
        worst = {}
        for name in PATHS:
            with forced(dev.ctx, name):
                worst[name] = bc.worst_ratio(dev.run_case(c), c["ref"])
    report(f"exact phases {shape} {span}", worst)


# ------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("name", list(PATHS))
def test_power_of_two_scaling_is_bit_exact(name):
    """The truncating split, the MFMA chains, k_sum_parts, the window and the FFT all commute with an exact scaling while nothing
    under- or overflows (the host test asserts that for these k): every path, bit for bit."""
    c = bc.scaling_case()
    with device(2, bc.MASKED) as dev, forced(dev.ctx, name):
        base = dev.run_case(c)
        assert bc.worst_ratio(base, c["ref"]) <= SPEC_TOL
        for k in bc.SCALE_K:
            got = dev.run(bc.scaled(c["X"], k), c["P"], c["dirs"], c["lam"])
            want = bc.scaled(base, k)
            differ = int(np.count_nonzero(bits(got) != bits(want)))
            assert differ == 0, f"{name}, k = {k}: {differ} of {got.size} outputs are not 2^k times the unscaled ones"


def test_all_ones_mantissa_operand():
    """Every part of X is +-(1 - 2^-24): the three dropped products of the bf16 x 3 kernels are as large as they get."""
    c = bc.ones_mantissa_case()
    with device(2, bc.MASKED) as dev:
        worst = {}
        for name in PATHS:
            with forced(dev.ctx, name):
                worst[name] = bc.worst_ratio(dev.run_case(c), c["ref"])
    report("all-ones mantissa", worst)


# ------------------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("which", ["index", "row"])
@pytest.mark.parametrize("E", bc.IMPULSE_E)
def test_impulse_operands_on_every_path(E, which):
    """X[f] is one 1 + 0j at (s0, e0): row s0 of the contraction is column e0 of W, so a k index fed to the wrong step, group,
    half-row or K-split part moves the whole frame.  E = 150 runs the masked kernels, E = 128 the FAST ones.  The GEMM paths get
    calls of at most two frames, where the planner splits K in four; the part boundaries of THIS device's plan are in the list."""
    cells = bc.index_list(E) if which == "index" else bc.row_list(E)
    num_cu = _lib.device_info(_lib.default_context().device)["num_cu"]
    for F in range(1, bc.GEMM_FRAMES_PER_CALL + 1):
        assert bc.plan(num_cu, F, bc.IMPULSE_S, E, bc.IMPULSE_T)[0] > 1
    assert {k for b in bc.part_boundaries(E, num_cu) for k in (b - 1, b)} <= {e for _, e in bc.index_list(E)}
    c = bc.impulse_case(E, cells)
    with device(10, (bc.IMPULSE_S, E, bc.IMPULSE_T)) as dev:
        worst = {}
        for name in PATHS:
            step = bc.GEMM_FRAMES_PER_CALL if name in GEMM_PATHS else 10
            with forced(dev.ctx, name):
                worst[name] = max(bc.worst_ratio(dev.run_case(c, slice(i, i + step)), c["ref"][i:i + step])
                                  for i in range(0, len(cells), step))
    report(f"impulses E={E} {which} list ({len(cells)} frames)", worst)


# ------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("shape", ["masked", "fast"])
@pytest.mark.parametrize("name", list(PATHS))
def test_a_frame_does_not_depend_on_its_batch(name, shape):
    """Frame f of a 5-frame call against a 1-frame call on that frame's X and P.  With the tile size forced the same kernel does
    the same arithmetic per output whatever the batch: bit patterns.  On the GEMM paths the K split is a function of the frame
    count AND of the device's CU count (bartlett_plan): where the two calls' plans agree -- at these shapes on 256 CUs they do,
    ksplit 1 at E = 37 and 2 at E = 64 for 1 and for 5 frames -- the bits agree too, where they differ the partial sums are
    grouped differently and the comparison is at the bar.  `default` chooses its kernel by the batch: at the bar."""
    dims = bc.MASKED if shape == "masked" else bc.FAST
    c = bc.dyadic_case(dims, "4 m", F=5, seed=31)
    num_cu = _lib.device_info(_lib.default_context().device)["num_cu"]
    exact = name in TILE_PATHS or (name in GEMM_PATHS and bc.plan(num_cu, 1, *dims) == bc.plan(num_cu, 5, *dims))
    with device(5, dims) as dev, forced(dev.ctx, name):
        batch = dev.run_case(c)
        assert bc.worst_ratio(batch, c["ref"]) <= SPEC_TOL
        for f in range(5):
            alone = dev.run_case(c, slice(f, f + 1))[0]
            if exact:
                assert np.array_equal(bits(alone), bits(batch[f])), f"{name}: frame {f} depends on its batch"
            else:
                assert np.abs(alone - batch[f]).max() <= SPEC_TOL * np.abs(c["ref"][f]).max()


@pytest.mark.parametrize("name", list(PATHS))
def test_a_non_finite_frame_stays_in_its_frame(name):
    """Frame 1 of X all NaN, all +inf, frame 1 of P all NaN: frames 0 and 2 keep their bits (a clamped or masked load that
    multiplied by zero where it should select would let the neighbour through), frame 1 is non-finite throughout."""
    c = bc.dyadic_case(bc.MASKED, "4 m", F=3, seed=41)
    with device(3, bc.MASKED) as dev, forced(dev.ctx, name):
        clean = dev.run_case(c)
        for what, value in (("X", np.nan), ("X", np.inf), ("P", np.nan)):
            X, P = c["X"].copy(), c["P"].copy()
            (X if what == "X" else P)[1] = value
            got = dev.run(X, P, c["dirs"], c["lam"])
            for f in (0, 2):
                assert np.array_equal(bits(got[f]), bits(clean[f])), f"{name}: frame {f} changed with frame 1 of {what} = {value}"
            assert not np.isfinite(got[1].real).any() and not np.isfinite(got[1].imag).any(), (name, what, value)


@pytest.mark.parametrize("name", list(PATHS))
def test_a_finite_extreme_stays_finite(name):
    """X[0, 35, E - 1] = 3e38, the last element of the last (partly filled) chunk, the one the clamped loads repeat: the float64
    reference is finite (2.4e37 at most), so is every output of frame 0, at the bar; frames 1 and 2 keep their bits."""
    c = bc.dyadic_case(bc.MASKED, "4 m", F=3, seed=41)
    X = c["X"].copy()
    X[0, 35, -1] = 3e38
    ref = bc.response(X[:1], bc.steering_exact(c["Pi"], c["Di"])[:1])
    assert np.isfinite(ref.astype(np.complex64)).all()
    with device(3, bc.MASKED) as dev, forced(dev.ctx, name):
        clean = dev.run_case(c)
        got = dev.run(X, c["P"], c["dirs"], c["lam"])
    assert np.isfinite(got[0]).all(), f"{name}: {np.count_nonzero(~np.isfinite(got[0]))} non-finite outputs"
    ratio = bc.worst_ratio(got[:1].astype(np.complex128), ref)
    print(f"3e38 element, {name}: {ratio:.2e} of the peak")
    assert ratio <= SPEC_TOL
    for f in (1, 2):
        assert np.array_equal(bits(got[f]), bits(clean[f])), f"{name}: frame {f} changed"


# ------------------------------------------------------------------------------------------------------------ E
def test_refused_arguments_leave_the_output_poisoned_and_a_good_call_follows():
    c = bc.dyadic_case(bc.MASKED, "4 m", F=2, seed=51)
    with device(2, bc.MASKED) as dev:
        dev.load(c["X"], c["P"], c["dirs"])
        dev.poison()
        bad = [dict(ctx=None), dict(X=None), dict(P=None), dict(dirs=None), dict(out=None), dict(n_frames=-1), dict(n_frames=65536),
               dict(S=0), dict(E=0), dict(T=0), dict(lam=0.0), dict(lam=-1.0), dict(lam=float("nan"))]
        for over in bad:
            assert dev.call(2, c["lam"], **over) == _lib.MMW_ERR_INVALID, over
            assert dev.ctx.lib.mmw_last_error(), over
            assert dev.untouched(), over
        with pytest.raises(ValueError):
            _lib.check(dev.call(2, c["lam"], S=0))
        # no frames: OK, nothing written
        assert dev.call(0, c["lam"]) == _lib.MMW_OK
        assert dev.untouched()
        # a good call afterwards on the same buffers
        assert bc.worst_ratio(dev.run_case(c), c["ref"]) <= SPEC_TOL


@pytest.mark.parametrize("case", list(bc.DEGENERATE))
def test_degenerate_shapes(case):
    """One sample (np.hanning(1) == [1.]: the bare contraction), two samples (the Hann window is all zeros: exact zeros, not
    NaN), one element, one direction, five directions (the padding of W's rows to a multiple of four)."""
    dims = bc.DEGENERATE[case]
    c = bc.dyadic_case(dims, "4 m", F=2, seed=61)
    with device(2, dims) as dev:
        worst = {}
        for name, opts in (("default", {}), ("tile kernels", {"MMW_BARTLETT_PATH": 1}), ("tiled GEMM", {"MMW_BARTLETT_PATH": 2})):
            try:
                for key, val in opts.items():
                    dev.ctx.set_option(key, val)
                got = dev.run_case(c)
            finally:
                for key in opts:
                    dev.ctx.set_option(key, None)
            if dims[0] == 2:
                assert not c["ref"].any() and not got.any(), f"{name}: {np.count_nonzero(got)} outputs are not zero"
                worst[name] = 0.0
            else:
                worst[name] = bc.worst_ratio(got, c["ref"])
    report(f"degenerate {case}", worst)
