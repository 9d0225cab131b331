"""nmx_field_gather / nmx_ppsnark_mem_oracles on the GPU, byte for byte against the definitions in Python integers
(tests/ppsnark_oracles_common.py; the lane bodies alone are checked on the CPU by tests/test_ppsnark_oracles_abi.py): all four fields, both
forms, host and HBM operands; the gather's shapes and refusals; the oracles at k = 1, 2 and 8 and the sizes either side of the host-top
boundary (128 chunk products), with one, two and three device levels and a size that is no multiple of the chunk; the edge contents;
NMX_E_ZERO for a zero T + r or W + r; a bad field id; overlapping HBM buffers; and ppsnark's prove from evaluation_oracles to the end of
prove_helper chained in HBM: gather -> oracles -> nmx_sumcheck_prove_ppsnark, accepted by the reference's verifier
(tests/ppsnark_sc_common.check_honest).
The reference of one (field, n) is computed ONCE for eight memories; k = 1 and k = 2 are its first one and two memories (the scalars are
the call's, so the same gamma and r serve every k), the Montgomery operands are the same values times 2^256."""
import ctypes
import functools
import random

import numpy as np
import pytest

from tests import fv_common as fc
from tests import ppsnark_oracles_common as oc
from tests import ppsnark_sc_common as pc

pytestmark = pytest.mark.gpu
R256 = oc.R256
SIZES = [1, 2, 127, 128, 129, 1000, 1025, 1 << 14]
# chunk products 2 k ceil(n / 8) against the host top's 128: k = 1: 127 -> 32 (no level above 0), 1000 -> 250 (one), 2^14 -> 4096 (two);
# k = 8: 1 -> 16, 127 / 128 -> 256, 129 -> 272, 2^14 -> 32768 (three levels above level 0: 4096, 512, 64)


@pytest.fixture(scope="module")
def L(nmx):
    from nova_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def fv(nmx):
    from nova_amd import fieldvec
    return fieldvec


def gpu(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def err_code(fn):
    from nova_amd.provider import NmxError
    with pytest.raises(NmxError) as e:
        fn()
    return e.value.code


# ---- the gather ---------------------------------------------------------------------------------------------------------------------------
GATHER_SHAPES = [(1, 1), (1, 300), (300, 1), (257, 1000), (1 << 14, 1 << 14)]


def gather_case(p, n_mem, n, seed):
    rng = random.Random(seed)
    mem = [rng.randrange(p) for _ in range(n_mem)]
    addr = [rng.randrange(n_mem) for _ in range(n)]
    addr[0], addr[-1] = n_mem - 1, 0                                    # cell n_mem - 1 and cell 0 are hit
    return mem, addr


def run_gather(fv, fid, mem_words, addr_words, device, mont):
    m, a = fc.vec(mem_words).copy(), fc.vec(addr_words).copy()
    m0, a0 = m.copy(), a.copy()
    out = fv.gather(fid, gpu(m) if device else m, gpu(a) if device else a, mont=mont)
    assert (m == m0).all() and (a == a0).all(), "host operands must be left untouched"
    return host(out)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("n_mem,n", GATHER_SHAPES)
def test_gather(fv, fid, n_mem, n):
    p = fc.FIELDS[fid]
    mem, addr = gather_case(p, n_mem, n, 100 * fid + n_mem + n)
    want = fc.vec(oc.gather(mem, addr))
    for mont in (False, True):
        for device in (True, False):
            got = run_gather(fv, fid, mem, oc.to_form(p, addr, mont), device, mont)      # mem is copied as it is: its form does not matter
            assert (got == want).all(), (mont, device)
    same = [n_mem // 2] * n                                             # every address equal
    assert (run_gather(fv, fid, mem, same, True, False) == fc.vec([mem[n_mem // 2]] * n)).all()


def test_gather_of_nothing(fv, L):
    from nova_amd import _lib
    mem = gpu(fc.vec([1, 2, 3]))
    out = fv.gather(1, mem, gpu(np.zeros((0, 32), np.uint8)))
    assert tuple(out.shape) == (0, 32)
    assert fv.gather(1, fc.vec([1, 2, 3]).copy(), np.zeros((0, 32), np.uint8)).shape == (0, 32)
    assert L.nmx_field_gather(1, mem.data_ptr(), 0, mem.data_ptr(), 0, _lib.SCALARS_DEVICE, mem.data_ptr() + 32) == 0    # n == 0: n_mem == 0 is fine


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("device", [True, False])
def test_gather_refuses_an_address_out_of_range_and_the_next_call_works(fv, device, mont):
    from nova_amd import _lib
    fid = 1
    p = fc.FIELDS[fid]
    n_mem, n = 257, 1000
    mem, addr = gather_case(p, n_mem, n, 9)
    want = fc.vec(oc.gather(mem, addr))
    form = R256 if mont else 1
    for j, bad in ((0, n_mem), (n - 1, n_mem), (500, n_mem + 1), (3, 1 << 32), (700, (1 << 32) + 5), (64, (1 << 224) + 1), (999, p - 1)):
        a = oc.to_form(p, addr, mont)
        a[j] = bad * form % p
        assert err_code(lambda: run_gather(fv, fid, mem, a, device, mont)) == _lib.E_ARG, (j, hex(bad))
        assert (run_gather(fv, fid, mem, oc.to_form(p, addr, mont), device, mont) == want).all()      # the next call on this thread works
    # words that are no field elements
    for w in (p, (1 << 256) - 1) + ((p + R256 % p,) if mont else ()):    # (Montgomery: p + 2^256 mod p reduces to the valid address 1)
        a = oc.to_form(p, addr, mont)
        a[17] = w
        assert err_code(lambda: run_gather(fv, fid, mem, a, device, mont)) == _lib.E_ARG, hex(w)
    assert (run_gather(fv, fid, mem, oc.to_form(p, addr, mont), device, mont) == want).all()


def test_gather_bad_field_and_overlap(fv, L):
    from nova_amd import _lib
    import torch
    mem, addr = gather_case(fc.FIELDS[1], 20, 10, 4)
    buf = gpu(np.concatenate([fc.vec(mem), fc.vec(addr), np.full((20, 32), 0x5a, np.uint8)]))     # mem [0, 20), addr [20, 30), free [30, 50)
    before = buf.cpu().numpy().copy()
    at = lambda i: buf.data_ptr() + 32 * i  # noqa: E731
    g = lambda out, field=1: L.nmx_field_gather(field, at(0), 20, at(20), 10, _lib.SCALARS_DEVICE, out)  # noqa: E731
    for bad in (4, -1):
        assert g(at(30), field=bad) == _lib.E_ARG and b"bad field id" in L.nmx_last_error()
    for out in (at(0), at(19), at(11), at(20), at(29), at(25)):
        assert g(out) == _lib.E_ARG and b"overlap" in L.nmx_last_error()
    assert L.nmx_field_gather(1, at(0), 20, at(20), 10, _lib.SCALARS_DEVICE | _lib.ASYNC, at(30)) == _lib.E_ARG
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == before).all()
    assert g(at(30)) == 0                                                 # adjacent, not overlapping: fine
    got = fc.ints(buf.cpu().numpy())
    assert got[30:40] == oc.gather(mem, addr) and got[:30] == mem + addr


# ---- the oracles ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shared_case(fid, n):
    """eight memories of n cells and their reference, computed once: (case, want as canonical integers)"""
    c = oc.random_case(fid, 8, n, seed=3 + fid)
    return c, c.want()


def operand_words(case, mont):
    """the case's four operand groups as byte arrays in the form `mont`, converted once per case"""
    cache = case.__dict__.setdefault("_words", {})
    if mont not in cache:
        cache[mont] = [[fc.vec(oc.to_form(case.p, v, mont)).copy() for v in grp] for grp in (case.mems, case.addrs, case.Ls, case.tss)]
    return cache[mont]


def run_oracles(fv, case, k, device, mont):
    """-> per memory the four outputs as (n, 32) byte arrays; the first k memories of the case"""
    p = case.p
    groups = [[v.copy() for v in grp[:k]] for grp in operand_words(case, mont)]
    before = [[v.copy() for v in grp] for grp in groups]
    args = [[gpu(v) for v in grp] for grp in groups] if device else groups
    out = fv.ppsnark_mem_oracles(case.fid, *args, fc.vec(oc.to_form(p, [case.gamma], mont)), fc.vec(oc.to_form(p, [case.r], mont)), mont=mont)
    assert all((a == b).all() for ga, gb in zip(groups, before) for a, b in zip(ga, gb)), "host operands must be left untouched"
    if device:
        assert all((host(a) == b).all() for ga, gb in zip(args, before) for a, b in zip(ga, gb)), "HBM inputs must be left untouched"
    return [tuple(host(x) for x in mem) for mem in out]


def expect(p, want, k, mont):
    return [tuple(fc.vec(oc.to_form(p, v, mont)) for v in mem) for mem in want[:k]]


def same(got, exp):
    return len(got) == len(exp) and all((a == b).all() for g, e in zip(got, exp) for a, b in zip(g, e))


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("n", SIZES)
def test_oracles(fv, fid, n):
    case, want = shared_case(fid, n)
    for mont in (False, True):
        for k in (1, 2, 8):
            exp = expect(case.p, want, k, mont)
            for device in (True, False):
                assert same(run_oracles(fv, case, k, device, mont), exp), (k, mont, device)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
def test_oracles_edge_contents(fv, fid):
    """mem entries 0 and p - 1, ts entries 0 and n, gamma = 0, gamma = p - 1 and r = 0 (tests/ppsnark_oracles_common.edge_cases)"""
    for n, k in ((1, 1), (2, 2), (129, 2), (1000, 8)):
        for case in oc.edge_cases(fid, k, n, seed=n + fid):
            want = case.want()
            for mont in (False, True):
                assert same(run_oracles(fv, case, k, True, mont), expect(case.p, want, k, mont)), (n, k, case.gamma == 0, case.r == 0, mont)
            assert same(run_oracles(fv, case, k, False, False), expect(case.p, want, k, False))


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("n,k", [(1, 1), (129, 2), (1025, 8)])
def test_a_zero_denominator_is_nmx_e_zero_and_the_next_call_works(fv, n, k, mont):
    """r = -(mem[m][j] gamma + j) makes exactly T_m[j] + r zero (j = 0 and n - 1, m = 0 and k - 1); r = -(L gamma + addr) a W element"""
    from nova_amd import _lib
    fid = 1
    case, want = shared_case(fid, n)
    p = case.p
    exp = expect(p, want, k, mont)
    zeros = [(-(case.mems[m][j] * case.gamma + j)) % p for m in {0, k - 1} for j in {0, n - 1}]
    zeros.append((-(case.Ls[k - 1][n // 2] * case.gamma + case.addrs[k - 1][n // 2])) % p)
    for device in (True, False):
        for r in zeros:
            bad = oc.Case(fid, case.k, n, case.mems, case.addrs, case.tss, case.gamma, r, Ls=case.Ls)
            with pytest.raises(oc.ZeroDenominator):
                oc.oracles(p, bad.mems[:k], bad.addrs[:k], bad.Ls[:k], bad.tss[:k], bad.gamma, r)
            assert err_code(lambda: run_oracles(fv, bad, k, device, mont)) == _lib.E_ZERO
            assert same(run_oracles(fv, case, k, device, mont), exp), "an error return, not a fault: the next call succeeds"


def test_oracles_bad_field_scalar_range_and_overlapping_hbm_buffers(fv, L):
    from nova_amd import _lib
    import torch
    fid, n, k = 1, 40, 2
    case = oc.random_case(fid, k, n, seed=77)
    want = case.want()
    p = case.p
    ins = np.concatenate([fc.vec(v) for grp in (case.mems, case.addrs, case.Ls, case.tss) for v in grp])       # vector j at [n j, n j + n), j < 8
    buf = gpu(np.concatenate([ins, np.full((9 * n, 32), 0x5a, np.uint8)]))                                     # outputs: vectors 8 .. 15, one spare
    before = buf.cpu().numpy().copy()
    at = lambda j, off=0: buf.data_ptr() + 32 * (n * j + off)  # noqa: E731
    arr = lambda *ptrs: (ctypes.c_void_p * 2)(*ptrs)  # noqa: E731
    gw, rw = fc.vec([case.gamma]).copy(), fc.vec([case.r]).copy()

    def o(field=fid, t=(at(8), at(9)), w=(at(10), at(11)), tinv=(at(12), at(13)), winv=(at(14), at(15)), gamma=gw, r=rw, flags=_lib.SCALARS_DEVICE):
        return L.nmx_ppsnark_mem_oracles(field, k, n, arr(at(0), at(1)), arr(at(2), at(3)), arr(at(4), at(5)), arr(at(6), at(7)), gamma.ctypes.data,
                                         r.ctypes.data, flags, arr(*t), arr(*w), arr(*tinv), arr(*winv))
    for bad in (4, -1):
        assert o(field=bad) == _lib.E_ARG and b"bad field id" in L.nmx_last_error()
    assert o(gamma=fc.vec([p]).copy()) == _lib.E_SCALAR_RANGE and o(r=fc.vec([p]).copy()) == _lib.E_SCALAR_RANGE
    assert o(flags=_lib.SCALARS_DEVICE | _lib.ASYNC) == _lib.E_ARG
    for kw in (dict(t=(at(0), at(9))), dict(winv=(at(14), at(7, 1))), dict(w=(at(10), at(3, n - 1))), dict(tinv=(at(12), at(8))),
               dict(t=(at(8), at(8, n - 1))), dict(winv=(at(14), at(13, 1)))):
        assert o(**kw) == _lib.E_ARG and b"overlap" in L.nmx_last_error(), kw
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == before).all(), "a refused call wrote something"
    assert o() == 0                                                       # adjacent vectors, nothing overlapping: fine
    got = fc.ints(buf.cpu().numpy())
    assert got[:8 * n] == fc.ints(ins), "HBM inputs must be left untouched"
    for m in range(k):
        for j, base in enumerate((8, 10, 12, 14)):
            assert got[n * (base + m):n * (base + m + 1)] == want[m][j], (m, j)
    assert got[16 * n:] == fc.ints(before[16 * n:])


def test_batch_invert_results_are_unchanged(fv):
    """nmx_field_batch_invert shares its levels above level 0 and its host top with the oracles (binv_levels): 2^14 elements, both forms"""
    fid = 1
    p = fc.FIELDS[fid]
    rng = random.Random(14)
    v = [rng.randrange(1, p) for _ in range(1 << 14)]
    inv = oc.inverses(p, v)
    assert (host(fv.batch_invert(fid, gpu(fc.vec(v)))) == fc.vec(inv)).all()
    vm = oc.to_form(p, v, True)
    assert (host(fv.batch_invert(fid, gpu(fc.vec(vm)), mont=True)) == fc.vec(oc.to_form(p, inv, True))).all()
    assert (fv.batch_invert(fid, fc.vec(v).copy()) == fc.vec(inv)).all()


# ---- prove, from evaluation_oracles to the end of prove_helper, in HBM ----------------------------------------------------------------------
@pytest.mark.parametrize("fid", [1, 2])
@pytest.mark.parametrize("l", [4, 10])
def test_gather_oracles_and_sumcheck_chained_in_hbm(fv, fid, l):
    """two random memories and address traces with ts from the trace; gather gives L_row / L_col, the oracle call the eight tables, and those
    with the other eight go into nmx_sumcheck_prove_ppsnark without leaving HBM.  check_honest (the reference's verifier, the sixteen finals,
    the brute-force round polynomials at l = 4) is given the same sixteen tables, read back once."""
    p = fc.FIELDS[fid]
    n = 1 << l
    rng = random.Random(5000 + 10 * fid + l)
    mems = [[rng.randrange(p) for _ in range(n)] for _ in range(2)]
    addrs = [[rng.randrange(n) for _ in range(n)] for _ in range(2)]
    tss = [oc.trace_counts(a, n) for a in addrs]
    mem_d, addr_d, ts_d = ([gpu(fc.vec(v)) for v in grp] for grp in (mems, addrs, tss))
    L_d = [fv.gather(fid, mem_d[g], addr_d[g]) for g in (0, 1)]                                   # evaluation_oracles
    assert [fc.ints(host(x)) for x in L_d] == [oc.gather(mems[g], addrs[g]) for g in (0, 1)]
    while True:                                                                                    # squeeze gamma, r (a seeded stand-in)
        gamma, r = rng.randrange(p), rng.randrange(p)
        try:
            oc.oracles(p, mems, addrs, [fc.ints(host(x)) for x in L_d], tss, gamma, r)
            break
        except oc.ZeroDenominator:
            continue
    orc = fv.ppsnark_mem_oracles(fid, mem_d, addr_d, L_d, ts_d, fc.vec([gamma]), fc.vec([r]))     # compute_oracles
    _rng, rho, ro, coeffs = pc._scalars(fid, l, 9, None, None)
    T = [None] * pc.NT
    for g in (0, 1):
        T[5 * g + pc.T_ROW], T[5 * g + pc.W_ROW], T[5 * g + pc.TINV_ROW], T[5 * g + pc.WINV_ROW] = orc[g]
        T[5 * g + pc.TS_ROW], T[pc.L_ROW + g] = ts_d[g], L_d[g]
    m = l // 2
    eqo = pc.eq_table(p, ro)
    rest = {pc.VAL: [rng.randrange(p) for _ in range(n)], pc.E: [rng.randrange(p) for _ in range(n)],
            pc.W: [rng.randrange(p) if i < (1 << m) else 0 for i in range(n)], pc.MASKED_EQ: [0 if i < (1 << m) else eqo[i] for i in range(n)]}
    for t, v in rest.items():
        T[t] = gpu(fc.vec(v))
    tables_host = [host(t).copy() for t in T]
    Lr, Lc = fc.ints(tables_host[pc.L_ROW]), fc.ints(tables_host[pc.L_COL])
    claims2 = [sum(a * b * c for a, b, c in zip(Lr, Lc, rest[pc.VAL])) % p, sum(x * y for x, y in zip(eqo, rest[pc.E])) % p]
    inst = pc.Instance(fid, l, tables_host, rho, ro, claims2, coeffs)

    def prove(fid_, _tables, rhos, r_outer, c2, co, tr):
        return fv.sumcheck_prove_ppsnark(fid_, [t.clone() for t in T], rhos, r_outer, c2, co, tr)  # the reference clones what it binds
    pc.check_honest(prove, inst)
