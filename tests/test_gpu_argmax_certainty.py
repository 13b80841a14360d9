"""The certainty decision of the float32 angle argmax kernels against an adversary, through mmw_angle_argmax_exact.

Inputs and labels: tests/argmax_certainty_cases.py (tests/test_argmax_certainty_cases_host.py proves them without a GPU).
The entry trusts d_cubes, d_l1 and d_rd: with an ALL-ZERO cube, crafted float32 cells in d_rd and crafted d_l1, a flagged
evaluation is refined from all-zero float64 cells -- a spectrum flat bit for bit, first maximum 0 -- and no winner of the
cases is output index 0.  So idx == 0 reads "flagged", idx == the exact winner "not flagged", anything else is wrong, and
the zeros must add up to n_refined.  One test per kernel launch_angle_argmax can pick (argmax_certainty_cases.DISPATCHES),
both shifts, the four frames in one call and each frame alone.  Asserted per evaluation:

    idx in {0, exact winner};  zeros == n_refined;  no must-flag evaluation unflagged;  no must-clear evaluation flagged;
    slots past counts[f] keep the poison.

Printed per dispatch (recorded in profiles/argmax_certainty_gpu_tests.log, not asserted): the label counts and how many
undecided evaluations the kernel cleared -- the measured tightness of the pairwise pass.

Teeth: with MMW_ARGMAX_BOUND_DIV = 8 (an eighth of the proof) every dispatch must leave at least one must-flag evaluation
unflagged.
"""
import numpy as np
import pytest

import argmax_certainty_cases as ac
from mmwave_radar_processing_amd import _lib

pytestmark = pytest.mark.gpu
POISON = -7


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


class Resident:
    def __init__(self, ctx, built):
        self.ctx, self.b = ctx, built
        b = built
        self.bufs = dict(cube=ctx.alloc(b.rd.nbytes), rd=ctx.alloc(b.rd.nbytes), l1=ctx.alloc(b.l1.nbytes), dets=ctx.alloc(b.dets.nbytes),
                         counts=ctx.alloc(b.counts.nbytes), idx=ctx.alloc(ac.F * ac.CAP * 4))
        self.bufs["cube"].zero()
        for key in ("rd", "l1", "dets", "counts"):
            self.bufs[key].upload(getattr(b, key))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for buf in self.bufs.values():
            buf.free()

    def run(self, shift, options, f0=0, n_frames=ac.F):
        """(n_refined, idx [n_frames][CAP]) of one call on frames f0 .. f0 + n_frames - 1."""
        ctx, q, d = self.ctx, self.bufs, self.b.dispatch
        q["idx"].upload(np.full((ac.F, ac.CAP), POISON, dtype=np.int32))
        arr, n_ant = _lib.int_array(self.b.ants)
        n_ref = _lib.C.c_int(-1)
        plane = ac.V * ac.S * ac.C * 8
        try:
            for key, value in options.items():
                ctx.set_option(key, value)
            rc = ctx.lib.mmw_angle_argmax_exact(ctx.handle, q["cube"].at(f0 * plane), q["l1"].at(f0 * ac.V * 4), q["rd"].at(f0 * plane),
                                                q["dets"].at(f0 * ac.CAP * 8), q["counts"].at(f0 * 4), q["idx"].at(f0 * ac.CAP * 4),
                                                n_frames, ac.V, ac.S, ac.C, ac.CAP, arr, n_ant, d.A, int(shift), _lib.C.byref(n_ref))
        finally:
            for key in options:
                ctx.set_option(key, None)
        assert rc == _lib.MMW_OK, f"{d.name}: A = {d.A}, n_ant = {d.n_ant}: return code {rc}"
        idx = q["idx"].download((ac.F, ac.CAP), np.int32)
        other = np.ones(ac.F, dtype=bool)
        other[f0:f0 + n_frames] = False
        assert np.all(idx[other] == POISON), f"{d.name}: a frame outside the call was written"
        return n_ref.value, idx[f0:f0 + n_frames]


def check(b, lab, idx, n_ref, f0, n_frames, tag):
    """The assertions of the module docstring on frames f0 .. ; returns (flagged [E'] bool, selection of the slots)."""
    sl = slice(f0 * ac.CAP, (f0 + n_frames) * ac.CAP)
    L, win, label = b.listed[sl], lab.winner[sl], lab.label[sl]
    got = idx.reshape(-1)
    assert np.all(got[~L] == POISON), f"{tag}: a slot past counts[f] was written"
    flagged = got == 0
    wrong = L & ~flagged & (got != win)
    assert not wrong.any(), (f"{tag}: {np.count_nonzero(wrong)} indices are neither 0 nor the exact winner, first slot "
                             f"{np.argmax(wrong)}: {got[np.argmax(wrong)]} != {win[np.argmax(wrong)]} ({b.kind[sl][np.argmax(wrong)]})")
    assert np.count_nonzero(flagged & L) == n_ref, f"{tag}: {np.count_nonzero(flagged & L)} zeros, n_refined {n_ref}"
    lax = L & (label == ac.MUST_FLAG) & ~flagged
    assert not lax.any(), (f"{tag}: {np.count_nonzero(lax)} must-flag evaluations came back unflagged, first slot {np.argmax(lax)} "
                           f"({b.kind[sl][np.argmax(lax)]}, l1 {b.profile[sl][np.argmax(lax)]}, rung {b.rung[sl][np.argmax(lax)]})")
    strict = L & (label == ac.MUST_CLEAR) & flagged
    assert not strict.any(), (f"{tag}: {np.count_nonzero(strict)} must-clear evaluations were flagged, first slot {np.argmax(strict)} "
                              f"({b.kind[sl][np.argmax(strict)]}, l1 {b.profile[sl][np.argmax(strict)]}, rung {b.rung[sl][np.argmax(strict)]})")
    return flagged


@pytest.mark.parametrize("name", [d.name for d in ac.DISPATCHES])
def test_certainty_decision(ctx, name, capsys):
    b = ac.build(name)
    d = b.dispatch
    with Resident(ctx, b) as res:
        for shift in (0, 1):
            lab = ac.labels(name, shift)
            tag = f"{name} ({d.kernel}) shift {shift}"
            n_ref, idx = res.run(shift, d.options)
            flagged = check(b, lab, idx, n_ref, 0, ac.F, tag)
            for f in range(ac.F):
                n1, idx1 = res.run(shift, d.options, f, 1)
                check(b, lab, idx1, n1, f, 1, f"{tag} frame {f} alone")
                np.testing.assert_array_equal(idx1[0], idx[f], err_msg=f"{tag}: frame {f} alone differs from the batch")
            # teeth: an eighth of the bound must let a must-flag evaluation through
            n8, idx8 = res.run(shift, dict(d.options, MMW_ARGMAX_BOUND_DIV=8))
            L = b.listed
            flagged8 = idx8.reshape(-1) == 0
            missed = np.count_nonzero(L & (lab.label == ac.MUST_FLAG) & ~flagged8)
            und = L & (lab.label == ac.UNDECIDED)
            nf, nc, nu = (np.count_nonzero(L & (lab.label == v)) for v in (ac.MUST_FLAG, ac.MUST_CLEAR, ac.UNDECIDED))
            with capsys.disabled():
                print(f"\n  {tag}: must-flag {nf} must-clear {nc} undecided {nu}; flagged {n_ref}; undecided cleared by the kernel "
                      f"{np.count_nonzero(und & ~flagged)} of {nu}; with the bound / 8: flagged {n8}, must-flag unflagged {missed}", end="")
            assert missed >= 1, f"{tag}: an eighth of the bound clears no must-flag evaluation: the cases are too blunt for this dispatch"


def test_one_antenna_flags_everything(ctx):
    """n_ant = 1: every spectrum is flat; every listed evaluation is flagged and answers 0."""
    b = ac.build(ac.FLAT_DISPATCH.name)
    with Resident(ctx, b) as res:
        for shift in (0, 1):
            n_ref, idx = res.run(shift, {})
            check(b, ac.labels(ac.FLAT_DISPATCH.name, shift), idx, n_ref, 0, ac.F, f"one antenna shift {shift}")
            assert n_ref == np.count_nonzero(b.listed)
