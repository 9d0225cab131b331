"""GPU: nmx_sumcheck_prove_ppsnark (RelaxedR1CSSNARK::prove_helper, src/spartan/ppsnark.rs:886-983) through the C ABI
(nova_amd.fieldvec's ctypes call) with CUDA tensors: random instances against the restatement of the reference in Python integers
(tests/ppsnark_sc_common.py_prove) byte for byte, honest instances through check_honest -- the reference's verifier, the final-claim
expression of ppsnark.rs:1566-1597, the sixteen final evaluations, the definition of the round polynomials at small sizes.  Every table
holds at most 2^13 elements: the smallest shapes at which each code path runs (the host tail alone up to 2^7; the hand-over and one-block
device passes at 2^8 / 2^9; two blocks' partials at 2^11; the change from first-half to last-half eq tables above the tail at 2^13).
Everything is exact."""
import random

import numpy as np
import pytest

from tests import fv_common as fc
from tests import ppsnark_sc_common as pc
from tests.spartan_common import le

pytestmark = pytest.mark.gpu


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def g_prove(fid, tables, rhos, r_outer, claims2, coeffs, tr, mont=False):
    from nova_amd import fieldvec as fv
    return fv.sumcheck_prove_ppsnark(fid, [dev(t) for t in tables], rhos, r_outer, claims2, coeffs, tr, mont=mont)


def both(fid, l, seed, prove=g_prove, force=None, honest=True, **kw):
    """a random instance against the restatement output for output; an honest one through check_honest and against the restatement"""
    rnd = pc.make_random(fid, l, seed, **kw)
    got = pc.run(prove, rnd, force)
    assert got == pc.run(pc.py_prove, rnd, force), "the HIP path and the restatement of the reference disagree on a random instance"
    if honest and "fill" not in kw:
        hon = pc.make_honest(fid, l, seed + 1, **kw)
        assert pc.check_honest(prove, hon, force) == pc.run(pc.py_prove, hon, force)
    return got


class option:
    """set a library option for a block and restore the default afterwards"""

    def __init__(self, name, value, default):
        self.name, self.value, self.default = name, value, default

    def __enter__(self):
        from nova_amd import _lib
        assert _lib.lib().nmx_set_option(self.name, self.value) == 0

    def __exit__(self, *_exc):
        from nova_amd import _lib
        assert _lib.lib().nmx_set_option(self.name, self.default) == 0


def all_on_device():
    return option(b"sc_host_tail", 0, 7)


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("l", [1, 2, 5, 8, 9])
def test_host_tail_hand_over_and_one_block_device_rounds(nmx, fid, l):
    both(fid, l, seed=700 + 10 * l)


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_two_blocks_of_partials(nmx, fid):
    """2^11: the first bind + sums pass has 512 indices -- the smallest case where partials of more than one block are added"""
    both(fid, 11, seed=810, honest=False)


def test_eight_blocks_and_the_last_half_eq_form_above_the_tail(nmx):
    """2^13 on BN254 Fr: round 6 is the first device round that uses eqR alone while the tables are still longer than the tail"""
    both(1, 13, seed=830, honest=False)


@pytest.mark.parametrize("l", [1, 2, 3, 5])
def test_every_round_on_the_device(nmx, l):
    """option sc_host_tail = 0: only the final values come to the host -- every round is a device pass (both eq forms), the len == 2
    hand-over and the sum-less last bind on one block included"""
    with all_on_device():
        got = [both(fid, l, seed=40 + l) for fid in (0, 1, 2, 3)]
    assert got == [pc.run(g_prove, pc.make_random(fid, l, 40 + l)) for fid in (0, 1, 2, 3)], "the same proof with the tail"


def _taus(fid, l, seed):
    p, rng = fc.FIELDS[fid], random.Random(seed)
    return [rng.randrange(p) for _ in range(l)], [rng.randrange(p) for _ in range(l)]


def test_fallbacks_on_the_device(nmx):
    """a zero rhos[j] / r_outer[j]: the third sum comes from one more pass over the group's high halves (sumcheck.rs:1085-1222) -- in a
    first-half round (both eq tables), in a last-half round (eqR alone), and for both eqs in the same round; with the challenge that
    makes the round after it start from a zero eq product (r = 1) as well"""
    fid, l = 1, 9
    rho, ro = _taus(fid, l, 55)
    z = lambda v, j: v[:j] + [0] + v[j + 1:]  # noqa: E731
    with all_on_device():
        for force in (None, {1: 1}):
            both(fid, l, seed=400, rhos=z(rho, 1), r_outer=ro, force=force)        # rhos[1] = 0: round 2 < first_half = 4
        both(fid, l, seed=410, rhos=rho, r_outer=z(ro, 6))                          # r_outer[6] = 0: round 7, the last half
        for force in (None, {3: 1}):
            both(fid, l, seed=420, rhos=z(rho, 3), r_outer=z(ro, 3), force=force)  # both zero in one round
        both(fid, l, seed=430, rhos=z(rho, 0), r_outer=z(ro, 8))                    # the first round (tables as the caller left them) and the last


def test_challenges_that_zero_a_running_eq_product(nmx):
    fid, l = 1, 9
    p = fc.FIELDS[fid]
    rho, ro = _taus(fid, l, 91)
    with all_on_device():
        for j in (1, 5):
            both(fid, l, seed=500 + j, rhos=rho, r_outer=ro, force={j: pc.zeroing_challenge(p, rho[j])})
            both(fid, l, seed=510 + j, rhos=rho, r_outer=ro, force={j: pc.zeroing_challenge(p, ro[j])})


def test_polling_and_synchronising_agree(nmx):
    inst = pc.make_random(1, 11, 5)
    with option(b"sc_poll_us", 0, 2000):
        got = pc.run(g_prove, inst)
    assert got == pc.run(g_prove, inst) == pc.run(pc.py_prove, inst)


@pytest.mark.parametrize("fid", [1, 3])
def test_montgomery_layout(nmx, fid):
    prove_m = pc.montgomery_wrapped(lambda *a: g_prove(*a, mont=True), fid)
    for l in (5, 9):
        both(fid, l, seed=9, prove=prove_m)
    inst = pc.make_random(fid, 11, 10)
    assert pc.run(prove_m, inst) == pc.run(g_prove, inst)


def test_host_arrays_give_the_same_proof_and_are_left_untouched(nmx):
    from nova_amd import fieldvec as fv
    kept = []

    def h_prove(fid, tables, rhos, r_outer, claims2, coeffs, tr):
        host = [t.copy() for t in tables]
        out = fv.sumcheck_prove_ppsnark(fid, host, rhos, r_outer, claims2, coeffs, tr)
        kept.append(all(np.array_equal(a, b) for a, b in zip(tables, host)))
        return out
    for l in (4, 9):
        inst = pc.make_honest(1, l, 21)
        assert pc.check_honest(h_prove, inst) == pc.run(g_prove, inst)
    assert kept == [True, True]


def test_all_entries_and_scalars_p_minus_one(nmx):
    """the lazy accumulators of all passes at their limb and value bounds (sumcheck_ppsnark.hpp kScPpsLazy)"""
    for fid in (0, 1, 2, 3):
        both(fid, 9, seed=62, fill=fc.FIELDS[fid] - 1)
        with all_on_device():
            both(fid, 9, seed=62, fill=fc.FIELDS[fid] - 1)


def test_errors_return_their_code_and_leave_the_tables_alone(nmx):
    import torch
    import nova_amd
    from nova_amd import _lib
    from nova_amd import fieldvec as fv
    fid, l = 1, 9
    n = 1 << l
    p = fc.FIELDS[fid]
    inst = pc.make_random(fid, l, 3)
    pool = dev(np.concatenate(inst.tables + [inst.tables[0]]))     # sixteen tables and a spare out of one allocation, so that overlaps can be built
    before = pool.clone()
    T = [pool[i * n:(i + 1) * n] for i in range(17)]
    calls = []

    def tr(_coeffs):
        calls.append(1)
        return le(7)

    def code(tables=None, rhos=inst.rhos, r_outer=inst.r_outer, claims2=inst.claims2, coeffs=inst.coeffs, transcript=tr, field=fid, untouched=True):
        with pytest.raises(nova_amd.NmxError) as e:
            fv.sumcheck_prove_ppsnark(field, tables or T[:16], rhos, r_outer, claims2, coeffs, transcript)
        torch.cuda.synchronize()
        if untouched:
            assert torch.equal(pool, before), "a refused call wrote the tables"
        return e.value.code
    assert code(tables=T[:9] + [T[2]] + T[10:16]) == _lib.E_ARG                                    # table 9 aliases table 2
    assert b"overlap" in _lib.lib().nmx_last_error()
    assert code(tables=T[:15] + [pool[14 * n + n // 2: 15 * n + n // 2]]) == _lib.E_ARG            # table 15 overlaps table 14 by half
    bad = lambda v, i: fc.vec(fc.ints(v)[:i] + [p] + fc.ints(v)[i + 1:]).copy()  # noqa: E731
    assert code(rhos=bad(inst.rhos, 4)) == _lib.E_SCALAR_RANGE
    assert code(r_outer=bad(inst.r_outer, 8)) == _lib.E_SCALAR_RANGE
    assert code(claims2=[inst.claims2[0], le(p)]) == _lib.E_SCALAR_RANGE
    assert code(coeffs=inst.coeffs[:8] + [le(2 ** 256 - 1)]) == _lib.E_SCALAR_RANGE
    for bad_id in (4, -1):
        assert code(field=bad_id) == _lib.E_ARG and b"bad field id" in _lib.lib().nmx_last_error()
    L = _lib.lib()
    import ctypes
    ptrs = (ctypes.c_void_p * 16)(*[t.data_ptr() for t in T[:16]])
    cb = fv.as_transcript(tr)
    c2, co = np.frombuffer(b"".join(inst.claims2), np.uint8).copy(), np.frombuffer(b"".join(inst.coeffs), np.uint8).copy()
    args = (inst.rhos.ctypes.data, inst.r_outer.ctypes.data, c2.ctypes.data, co.ctypes.data)
    assert L.nmx_sumcheck_prove_ppsnark(fid, l, ptrs, *args, _lib.SCALARS_DEVICE | 8, cb, None, None, None, None) == _lib.E_ARG   # an unknown flag
    assert L.nmx_sumcheck_prove_ppsnark(fid, l, None, *args, _lib.SCALARS_DEVICE, cb, None, None, None, None) == _lib.E_ARG      # NULL tables
    assert L.nmx_sumcheck_prove_ppsnark(fid, l, ptrs, None, *args[1:], _lib.SCALARS_DEVICE, cb, None, None, None, None) == _lib.E_ARG
    assert L.nmx_sumcheck_prove_ppsnark(fid, l, ptrs, *args, _lib.SCALARS_DEVICE, _lib.TRANSCRIPT_FN(), None, None, None, None) == _lib.E_ARG
    assert L.nmx_sumcheck_prove_ppsnark(fid, 31, ptrs, *args, _lib.SCALARS_DEVICE, cb, None, None, None, None) != 0
    torch.cuda.synchronize()
    assert torch.equal(pool, before) and not calls, "a refused call reached the tables or the transcript"
    want = pc.run(pc.py_prove, inst)
    with all_on_device():          # every round on the device: round 3's failure comes after two bind + sums passes
        def fails_in_round_3(_coeffs):
            calls.append(1)
            if len(calls) == 3:
                raise RuntimeError("transcript refused")
            return le(7)
        assert code(transcript=fails_in_round_3, untouched=False) == _lib.E_ARG and len(calls) == 3
        assert pc.run(g_prove, inst) == want, "the call after a failed callback, on the same thread"
        del calls[:]

        def too_big_in_round_3(_coeffs):
            calls.append(1)
            return b"\xff" * 32 if len(calls) == 3 else le(7)
        assert code(transcript=too_big_in_round_3, untouched=False) == _lib.E_SCALAR_RANGE and len(calls) == 3
        assert pc.run(g_prove, inst) == want, "the call after a challenge >= p, on the same thread"
    pool.copy_(before)             # (the two failed proofs above had bound the tables twice)
    torch.cuda.synchronize()
    assert code(transcript=lambda c: b"\xff" * 32) == _lib.E_SCALAR_RANGE      # round 1: only the sums passes have run, nothing is written
    assert pc.run(g_prove, inst) == want


def test_two_threads_prove_different_instances_at_once(nmx):
    import threading
    jobs = [pc.make_random(1, 11, 201), pc.make_random(3, 9, 202)]
    want = [pc.run(pc.py_prove, j) for j in jobs]
    errs = []

    def prover(i):
        try:
            for _ in range(2):
                assert pc.run(g_prove, jobs[i]) == want[i], i
        except Exception as e:   # noqa: BLE001 -- reported by the main thread
            errs.append((i, repr(e)))
    ths = [threading.Thread(target=prover, args=(i,)) for i in range(len(jobs))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs
