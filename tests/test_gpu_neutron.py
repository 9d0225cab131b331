"""nmx_pow_split_evals / nmx_neutron_fold_sums / nmx_neutron_relation_sum / nmx_neutron_fold_witness on the GPU, bit for bit against
tests/neutron_common.py (the definitions in Python integers, itself checked on the CPU by tests/test_neutron_abi.py): all four fields,
canonical and Montgomery words, host and HBM operands, shapes from (1, 1) to (512, 256), every grid the option neutron_max_blocks forces,
the edge contents (0, p - 1, words at and above p, the four special rho, a zero running instance, equal instances), NMX_ASYNC, and one
folding step of neutron::NIFS::prove chained in HBM whose check is the reference's execute_sequence invariant (nifs.rs:366-435), not the
restatement of the sums."""
import random

import numpy as np
import pytest

from tests import fv_common as fc
from tests import neutron_common as nc

pytestmark = pytest.mark.gpu
FIELDS = sorted(fc.FIELDS)


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


def ints(x):
    return fc.ints(np.frombuffer(x, np.uint8)) if isinstance(x, (bytes, bytearray)) else (fc.ints(host(x)) if len(x) else [])


def place(vs, device):
    return [gpu(fc.vec(v)) if device else fc.vec(v).copy() for v in vs]


def run_fold_sums(fv, case, mont, device):
    return ints(fv.neutron_fold_sums(case.fid, case.left, case.right, *place(case.vecs, device), fc.vec(nc.words(case.p, [case.rho], mont)), mont=mont))


def run_relation(fv, case, mont, device, which=1):
    return ints(fv.neutron_relation_sum(case.fid, case.left, case.right, *place(case.vecs[4:] if which == 2 else case.vecs[:4], device), mont=mont))


def check_case(fv, case, mont, device):
    p = case.p
    assert run_fold_sums(fv, case, mont, device) == nc.words(p, case.want_fold(mont), mont), (case.name, case.fid, case.left, case.right, mont, device)
    assert run_relation(fv, case, mont, device) == nc.words(p, [case.want_relation(mont)], mont), (case.name, case.fid, case.left, case.right, mont, device)


# ---- the two sums ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("fid", FIELDS)
def test_sums_small_shapes(fv, fid, mont):
    for left, right in nc.SMALL_SHAPES:
        case = nc.random_case(fid, left, right)
        check_case(fv, case, mont, True)
        check_case(fv, case, mont, False)


@pytest.mark.parametrize("left,right", nc.LARGE_SHAPES)
@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("fid", FIELDS)
def test_sums_large_shapes(fv, fid, mont, left, right):
    """more tiles than one block takes, rows of two and four tiles"""
    case = nc.random_case(fid, left, right)
    check_case(fv, case, mont, True)
    check_case(fv, case, mont, False)


@pytest.mark.parametrize("left,right", [(8, 4), (65, 7), (256, 256)])
def test_sums_do_not_depend_on_the_forced_grid(fv, L, left, right):
    """(65, 7) is seven tiles, two blocks by size; (256, 256) 64 blocks: one block walks every tile, three leave an uneven share"""
    try:
        for fid in (1, 2):
            case = nc.random_case(fid, left, right)
            want = nc.words(case.p, case.want_fold(False), False)
            for opt in (1, 2, 3, 5000, 0):
                assert L.nmx_set_option(b"neutron_max_blocks", opt) == 0
                assert run_fold_sums(fv, case, False, True) == want, (fid, opt)
                assert run_relation(fv, case, False, True) == nc.words(case.p, [case.want_relation(False)], False), (fid, opt)
    finally:
        assert L.nmx_set_option(b"neutron_max_blocks", 0) == 0


@pytest.mark.parametrize("fid", FIELDS)
def test_sums_edge_contents(fv, fid):
    for left, right in ((3, 5), (65, 7)):
        for case in nc.edge_cases(fid, left, right):
            check_case(fv, case, False, True)
            check_case(fv, case, True, True)
    for case in nc.edge_cases(fid, 8, 4):
        check_case(fv, case, fid % 2 == 0, False)


def test_a_challenge_out_of_range_writes_nothing(fv, L):
    from nova_amd import _lib
    p = fc.FIELDS[1]
    case = nc.random_case(1, 3, 5)
    vs = place(case.vecs, True)
    out = np.full(160, 0xA5, np.uint8)
    for rho in (p, p + 1, (1 << 256) - 1):
        r = fc.vec([rho]).copy()
        assert L.nmx_neutron_fold_sums(1, 3, 5, *[v.data_ptr() for v in vs], r.ctypes.data, _lib.SCALARS_DEVICE, out.ctypes.data) == _lib.E_SCALAR_RANGE
        assert (out == 0xA5).all()
    w1, w2 = gpu(fc.vec(case.vecs[1])), gpu(fc.vec(case.vecs[2]))
    before = host(w1).copy()
    r = fc.vec([p]).copy()
    assert L.nmx_neutron_fold_witness(1, w1.data_ptr(), w2.data_ptr(), 15, None, None, 0, r.ctypes.data, _lib.SCALARS_DEVICE, w1.data_ptr(), None) == _lib.E_SCALAR_RANGE
    fv.sync()
    assert (host(w1) == before).all()


# ---- the witness fold -----------------------------------------------------------------------------------------------------------------
LENGTHS = ((0, 1), (1, 0), (63, 64), (64, 65), (65, 1000), (1000, 63), (1, 1), (0, 65))


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("fid", FIELDS)
def test_fold_witness(fv, fid, mont):
    p, rng = fc.FIELDS[fid], random.Random(11 * fid + mont)
    word = lambda: rng.choice([0, p - 1, p, p + 1, nc.R256 - 1]) if rng.random() < 0.15 else rng.randrange(p)  # noqa: E731
    for n_w, n_e in LENGTHS:
        vs = [[word() for _ in range(m)] for m in (n_w, n_w, n_e, n_e)]
        vals = [nc.values(p, v, mont) for v in vs]
        for r_b in (0, 1, p - 1, rng.randrange(p)):
            want = tuple(nc.words(p, x, mont) for x in nc.fold_witness(p, *vals, r_b))
            rw = fc.vec(nc.words(p, [r_b], mont))
            for device in (True, False):
                ops = place(vs, device)
                w, e = fv.neutron_fold_witness(fid, *ops, rw, mont=mont)
                assert (ints(w), ints(e)) == want, (n_w, n_e, r_b, device)
                assert [ints(o) for o in ops] == vs, "out of place: the operands stay as they were"
                w, e = fv.neutron_fold_witness(fid, *ops, rw, mont=mont, inplace=True)        # over w1 and e1
                assert (ints(w), ints(e)) == want, (n_w, n_e, r_b, device, "in place")
                if device:
                    assert (ints(ops[0]), ints(ops[2])) == want and [ints(ops[1]), ints(ops[3])] == [vs[1], vs[3]]


# ---- the pow tables -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("fid", FIELDS)
def test_pow_split_evals(fv, fid, mont):
    p, rng = fc.FIELDS[fid], random.Random(13 * fid + mont)
    for left, right in ((1, 1), (2, 1), (1, 2), (3, 5), (1024, 1024), (2048, 1024)):
        for tau in (0, 1, p - 1, rng.randrange(p)):
            want = nc.words(p, nc.pow_split_evals(p, tau, left, right), mont)
            tw = fc.vec(nc.words(p, [tau], mont))
            assert ints(fv.pow_split_evals(fid, tw, left, right, mont=mont, device="cuda")) == want, (left, right, tau, "HBM")
            assert ints(fv.pow_split_evals(fid, tw, left, right, mont=mont)) == want, (left, right, tau, "host")


# ---- NMX_ASYNC ------------------------------------------------------------------------------------------------------------------------
def test_async_forms_are_ordered_and_complete_at_sync(fv):
    """pow tables and two folds enqueued without a wait, each reading what the one before wrote; a synchronous sum behind them"""
    fid, left, right = 1, 65, 7
    p = fc.FIELDS[fid]
    case = nc.random_case(fid, left, right)
    tau, r1, r2 = 12345, 777, p - 2
    E = fv.pow_split_evals(fid, fc.vec([tau]), left, right, device="cuda", async_=True)
    ops = place(case.vecs, True)
    w, e = fv.neutron_fold_witness(fid, ops[1], ops[5], ops[0], E, fc.vec([r1]), async_=True)           # e = E1 + r1 (pow - E1)
    w2, e2 = fv.neutron_fold_witness(fid, w, ops[5], e, E, fc.vec([r2]), async_=True, inplace=True)     # over w and e
    Ev = nc.pow_split_evals(p, tau, left, right)
    wa, ea = nc.fold_witness(p, case.vecs[1], case.vecs[5], case.vecs[0], Ev, r1)
    wb, eb = nc.fold_witness(p, wa, case.vecs[5], ea, Ev, r2)
    got = ints(fv.neutron_relation_sum(fid, left, right, e2, w2, ops[2], ops[3]))                       # synchronous: ordered behind the three
    assert got == [nc.relation_sum(p, left, right, eb, wb, case.vecs[2], case.vecs[3])]
    fv.sync()
    assert ints(E) == Ev and (ints(w2), ints(e2)) == (wb, eb) and w2 is w and e2 is e


# ---- one folding step, checked by the protocol's own invariant ------------------------------------------------------------------------------
def csr_times(p, csr, z):
    ip, ix, dt = csr
    vals = fc.ints(dt)
    return [sum(vals[k] * z[int(ix[k])] for k in range(int(ip[i]), int(ip[i + 1]))) % p for i in range(len(ip) - 1)]


def test_one_folding_step_keeps_the_folded_relation(fv):
    """neutron::NIFS::prove (nifs.rs:200-289) over a 64-row R1CS on BN254 Fr: a satisfying z2 (T2 = 0), an arbitrary running (z1, E1) whose
    claim T1 is its own relation sum; pow tables, both multiply_vec products, the five sums and the fold on the device, the O(1) algebra here.
    The folded witness must satisfy the folded instance: its relation sum is T_out = poly(r_b) / eq(rho, r_b) -- execute_sequence's
    is_sat after every step (nifs.rs:366-435)."""
    from tests import r1cs_sat_common as S
    fid, left, right = 1, 8, 8
    p, rng = fc.FIELDS[fid], random.Random(2024)
    inst = S.make_strict(fid, left * right, 40, n_io=2, seed=23)
    z2 = fc.ints(inst.z())
    assert inst.bad_rows()[0] == 0 and z2[inst.n_w] == 1
    z1 = [rng.randrange(p) for _ in range(inst.cols)]
    E1 = [rng.randrange(p) for _ in range(left + right)]
    mats = [fv.SparseMatrix(fid, ip, ix, dt, inst.cols) for ip, ix, dt in inst.csr]
    try:
        tau, rho, r_b = (rng.randrange(p) for _ in range(3))
        assert nc.eq(p, rho, r_b) != 0
        # the running claim, computed here from the matrices themselves
        T1 = nc.relation_sum(p, left, right, E1, *[csr_times(p, m, z1) for m in inst.csr])
        T = (1 - rho) * T1 % p                                                     # T2 = 0
        # device steps
        z1_d, z2_d, E1_d = gpu(fc.vec(z1)), gpu(fc.vec(z2)), gpu(fc.vec(E1))
        E2_d = fv.pow_split_evals(fid, fc.vec([tau]), left, right, device="cuda", async_=True)
        abc1 = fv.multiply_vec_many(mats, z1_d, async_=True)
        abc2 = fv.multiply_vec_many(mats, z2_d, async_=True)
        o = ints(fv.neutron_fold_sums(fid, left, right, E1_d, *abc1, E2_d, *abc2, fc.vec([rho])))
        z_d, E_d = fv.neutron_fold_witness(fid, z1_d, z2_d, E1_d, E2_d, fc.vec([r_b]), async_=True)
        # host algebra
        poly = nc.from_evals(p, [o[0], (T - o[0]) % p, o[1], o[2], o[3], o[4]])
        assert (nc.poly_eval(p, poly, 0) + nc.poly_eval(p, poly, 1)) % p == T
        T_out = nc.poly_eval(p, poly, r_b) * pow(nc.eq(p, rho, r_b), -1, p) % p
        # the folded instance-witness pair
        abc = fv.multiply_vec_many(mats, z_d, async_=True)
        assert ints(fv.neutron_relation_sum(fid, left, right, E_d, *abc)) == [T_out]
        # instance 2 alone is satisfied under ANY E: its relation sum is zero, which is what T2 = 0 claims
        assert ints(fv.neutron_relation_sum(fid, left, right, E2_d, *abc2)) == [0]
        fv.sync()
        assert ints(E2_d) == nc.pow_split_evals(p, tau, left, right)
    finally:
        for m in mats:
            m.close()
