"""nmx_sumcheck_prove_ppsnark without a GPU.  (1) The entry point is declared, exported and bound in Python / C++ / Rust, and its
argument errors return with no device present.  (2) The host tail (sc_tail_rounds_ppsnark, nova_amd/csrc/sc_host.hpp) compiled with g++
as a complete prover over sixteen host tables (tests/cpp/sc_ppsnark_host_test.cpp) equals the plain restatement of the reference in
Python integers (tests/ppsnark_sc_common.py_prove) output for output on random instances, and passes check_honest -- the reference's
verifier, the sixteen final evaluations, the definition of every round polynomial -- on honest ones, the tau = 0 fallbacks and the
eq-zeroing challenges included.  (3) The lane bodies of all seven new kernels (nova_amd/csrc/sumcheck_ppsnark.hpp) run thread by
thread under tests/host_emul/simt.hpp with limb bounds asserted, against big-integer sums.  What the emulation does NOT run: the block
reductions (shuffles), the mailbox sum (k_sum_partials_mail) and the host half of the device rounds; tests/test_gpu_sumcheck_ppsnark.py
covers those."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import cref
from tests import fv_common as fc
from tests import ppsnark_sc_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
PARAMS = ["int field_id", "size_t num_rounds", "void* const* tables", "const void* rhos", "const void* r_outer", "const void* claims2",
          "const void* coeffs9", "uint32_t flags", "nmx_transcript_fn transcript", "void* ctx", "uint8_t* out_polys", "uint8_t* out_r",
          "uint8_t* out_finals"]
ENUM = ["NMX_PPS_T_ROW", "NMX_PPS_TINV_ROW", "NMX_PPS_W_ROW", "NMX_PPS_WINV_ROW", "NMX_PPS_TS_ROW", "NMX_PPS_T_COL", "NMX_PPS_TINV_COL",
        "NMX_PPS_W_COL", "NMX_PPS_WINV_COL", "NMX_PPS_TS_COL", "NMX_PPS_L_ROW", "NMX_PPS_L_COL", "NMX_PPS_VAL", "NMX_PPS_E", "NMX_PPS_W",
        "NMX_PPS_MASKED_EQ", "NMX_PPS_TABLES"]


@pytest.fixture(scope="module")
def L():
    from nova_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- (1) the surface -------------------------------------------------------------------------------------------------------------
def test_header_declares_library_exports_and_python_binds_the_same_types(L):
    from nova_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nova_mi355x.h")).read()
    m = re.search(r"int nmx_sumcheck_prove_ppsnark\(([^;]*)\);", hdr)
    assert m, "the header does not declare nmx_sumcheck_prove_ppsnark"
    plist = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)               # `/* 16 */` and `/* 16 x 32 */` annotate two parameters
    assert [x.strip() for x in re.sub(r"\s+", " ", plist).split(",")] == PARAMS
    assert hasattr(L, "nmx_sumcheck_prove_ppsnark")
    ctype_of = lambda d: (ctypes.c_int if d.startswith("int ") else ctypes.c_size_t if d.startswith("size_t") else ctypes.c_uint32  # noqa: E731
                          if d.startswith("uint32_t") else _lib.TRANSCRIPT_FN if d.startswith("nmx_transcript_fn") else ctypes.c_void_p)
    assert list(L.nmx_sumcheck_prove_ppsnark.argtypes) == [ctype_of(d) for d in PARAMS]
    em = re.search(r"enum \{\s*(NMX_PPS_T_ROW[^}]*)\}", hdr)
    assert em and [re.sub(r"\s*=.*", "", x.strip()) for x in em.group(1).split(",")] == ENUM and "NMX_PPS_TABLES = 16" in em.group(1)
    doc = hdr.split("int nmx_sumcheck_prove_ppsnark(")[0].rsplit("/* nmx_sumcheck_prove_ppsnark ==", 1)[1]
    for needle in ("ppsnark.rs:886-983", "ppsnark.rs:520-670", "ppsnark.rs:725-786", "ppsnark.rs:293-325", "sumcheck.rs:356-379", "sumcheck.rs:900-1037",
                   "sumcheck.rs:416-443", "sumcheck.rs:1039-1080", "sumcheck.rs:384-407", "sumcheck.rs:1085-1222", "NMX_E_ARG", "NMX_E_SCALAR_RANGE",
                   "BOUND IN PLACE", "overlap", "sc_host_tail", "sc_poll_us", "do NOT affect"):
        assert needle in doc, needle
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    assert "pub fn nmx_sumcheck_prove_ppsnark(" in ffi and "pub const NMX_PPS_MASKED_EQ" in ffi, "ffi.rs: regenerate with scripts/gen_rust_sys.py"


def test_python_and_cpp_wrappers_exist():
    import inspect
    from nova_amd import fieldvec as fv
    assert list(inspect.signature(fv.sumcheck_prove_ppsnark).parameters) == ["field", "tables", "rhos", "r_outer", "claims2", "coeffs", "transcript",
                                                                             "mont", "ctx"]
    assert len(fv.PPS_TABLES) == 16
    hpp = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read()
    assert "static SumcheckProof prove_ppsnark(const std::vector<std::vector<Scalar>>& tables" in hpp
    assert "inline Proof prove_ppsnark(int field" in hpp.split("namespace resident {")[1]
    z, cb = fc.vec([0, 0]), (lambda c: bytes(32))
    with pytest.raises(AssertionError, match="sixteen tables"):
        fv.sumcheck_prove_ppsnark(1, [z] * 15, fc.vec([1]), fc.vec([1]), [bytes(32)] * 2, [bytes(32)] * 9, cb)


def test_argument_errors_need_no_device_and_touch_nothing(L):
    from nova_amd import _lib
    fid, l = 1, 3
    p = fc.FIELDS[fid]
    n = 1 << l
    cb = _lib.TRANSCRIPT_FN(lambda *_a: 1)
    big = np.ascontiguousarray(fc.rand_vec(fid, 17 * n, 3).copy())
    before = big.copy()
    tab = lambda i, off=0: big.ctypes.data + 32 * (n * i + off)  # noqa: E731
    good = [tab(i) for i in range(16)]

    def call(tables=good, rhos=(2, 3, 4), r_outer=(5, 6, 7), claims2=(1, 2), coeffs=(1, 2, 3, 4, 5, 6, 7, 8, 9), field=fid, cb_=cb, nr=l, flags=0, null=None):
        arr = (ctypes.c_void_p * 16)(*tables) if tables is not None else None
        v = {k: fc.vec(list(x)).copy() for k, x in dict(rhos=rhos, r_outer=r_outer, claims2=claims2, coeffs=coeffs).items()}
        ptr = {k: (None if k == null else a.ctypes.data) for k, a in v.items()}
        return L.nmx_sumcheck_prove_ppsnark(field, nr, arr, ptr["rhos"], ptr["r_outer"], ptr["claims2"], ptr["coeffs"], flags, cb_, None, None, None, None)
    assert call(tables=None) == _lib.E_ARG                                          # NULL tables
    for t in (0, 7, 15):
        assert call(tables=good[:t] + [None] + good[t + 1:]) == _lib.E_ARG          # a NULL entry
    for name in ("rhos", "r_outer", "claims2", "coeffs"):
        assert call(null=name) == _lib.E_ARG, name                                  # a NULL scalar pointer
    assert call(cb_=_lib.TRANSCRIPT_FN()) == _lib.E_ARG                             # null callback
    assert call(tables=good[:9] + [tab(2)] + good[10:]) == _lib.E_ARG               # table 9 aliases table 2
    assert b"overlap" in L.nmx_last_error()
    assert call(tables=good[:15] + [tab(14, n // 2)]) == _lib.E_ARG                 # a table overlapping another by half
    assert b"overlap" in L.nmx_last_error()
    assert call(field=4) == _lib.E_ARG and call(field=-1) == _lib.E_ARG
    assert b"bad field id" in L.nmx_last_error()
    for bad in (2, 8, 1 << 31, 3 | 4 | 16):
        assert call(flags=bad) == _lib.E_ARG, bad                                   # a flag other than NMX_SCALARS_MONT / NMX_SCALARS_DEVICE
    assert call(nr=31) != 0 and call(nr=64) != 0
    assert call(rhos=(2, p, 4)) == _lib.E_SCALAR_RANGE
    assert call(r_outer=(5, 6, p + 1)) == _lib.E_SCALAR_RANGE
    assert call(claims2=(p, 2)) == _lib.E_SCALAR_RANGE and call(claims2=(1, 2 ** 256 - 1)) == _lib.E_SCALAR_RANGE
    for i in range(9):
        co = [1] * 9
        co[i] = p
        assert call(coeffs=co) == _lib.E_SCALAR_RANGE, i
    assert (big == before).all()


# ---- (2) the host prover ------------------------------------------------------------------------------------------------------------
_hlib = None


def hscp():
    global _hlib
    if _hlib is None:
        so = os.path.join(ROOT, "tests", "cpp", "libsc_ppsnark_host_test.so")
        src = os.path.join(ROOT, "tests", "cpp", "sc_ppsnark_host_test.cpp")
        deps = [src] + [os.path.join(CSRC, f) for f in ("sc_host.hpp", "host_fp4.hpp", "fp.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
        _hlib = ctypes.CDLL(so)
    return _hlib


def h_prove(fid, tables, rhos, r_outer, claims2, coeffs, tr, mont=0):
    keep = [np.ascontiguousarray(t) for t in tables]
    before = [t.copy() for t in keep]
    ptrs = (ctypes.c_void_p * 16)(*[t.ctypes.data for t in keep])
    rh, ro = np.ascontiguousarray(rhos), np.ascontiguousarray(r_outer)
    nr = rh.size // 32
    c2, co = np.frombuffer(b"".join(claims2), np.uint8).copy(), np.frombuffer(b"".join(coeffs), np.uint8).copy()
    polys, r, fin = np.zeros(128 * max(nr, 1), np.uint8), np.zeros(32 * max(nr, 1), np.uint8), np.zeros(32 * 16, np.uint8)
    cb = cref.make_transcript(tr)
    vp = ctypes.c_void_p
    rc = hscp().hscp_prove_ppsnark(fid, mont, ctypes.c_size_t(nr), ptrs, vp(rh.ctypes.data), vp(ro.ctypes.data), vp(c2.ctypes.data), vp(co.ctypes.data),
                                   cb, None, vp(polys.ctypes.data), vp(r.ctypes.data), vp(fin.ctypes.data))
    assert rc == 0
    assert all((a == b).all() for a, b in zip(keep, before))
    pb, rb, fb = polys.tobytes(), r.tobytes(), fin.tobytes()
    return ([[pb[128 * j + 32 * i: 128 * j + 32 * i + 32] for i in range(4)] for j in range(nr)], [rb[32 * j: 32 * j + 32] for j in range(nr)],
            [fb[32 * t: 32 * t + 32] for t in range(16)])


def both(fid, l, seed, prove=h_prove, force=None, **kw):
    """a random instance against the restatement output for output, an honest one through check_honest (and against the restatement too)"""
    rnd = pc.make_random(fid, l, seed, **kw)
    got = pc.run(prove, rnd, force)
    assert got == pc.run(pc.py_prove, rnd, force), "the prover and the restatement of the reference disagree on a random instance"
    if "fill" not in kw:
        hon = pc.make_honest(fid, l, seed + 1, **kw)
        assert pc.check_honest(prove, hon, force) == pc.run(pc.py_prove, hon, force)
    return got


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("l", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_host_prover(fid, l):
    both(fid, l, seed=1000 + 10 * l)


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("l", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_host_prover_montgomery_words(fid, l):
    both(fid, l, seed=50 + l, prove=pc.montgomery_wrapped(lambda *a: h_prove(*a, mont=1), fid))


def test_the_restatement_itself_passes_the_verifier():
    for fid, l in ((1, 0), (1, 4), (2, 3)):
        pc.check_honest(pc.py_prove, pc.make_honest(fid, l, 9))


@pytest.mark.parametrize("l", [3, 6])
def test_fallback_when_a_tau_is_zero(l):
    fid = 1
    p = fc.FIELDS[fid]
    rng = random.Random(55 + l)
    base_rho, base_ro = [rng.randrange(p) for _ in range(l)], [rng.randrange(p) for _ in range(l)]
    for j in (0, l // 2, l - 1):               # the first round, a middle round, the last round
        zr, zo = list(base_rho), list(base_ro)
        zr[j], zo[j] = 0, 0
        for force in (None, {j: 1}):
            both(fid, l, seed=400 + j, rhos=zr, r_outer=base_ro, force=force)        # rhos[j] = 0 alone: claims 2-5 fall back
            both(fid, l, seed=410 + j, rhos=base_rho, r_outer=zo, force=force)       # r_outer[j] = 0 alone: claim 7 falls back
            both(fid, l, seed=420 + j, rhos=zr, r_outer=zo, force=force)             # both in the same round
    both(fid, l, seed=77, rhos=[0] * l, r_outer=[0] * l)


@pytest.mark.parametrize("fid", [1, 3])
def test_a_challenge_that_zeroes_a_running_eq_product(fid):
    """after r_j = (1 - tau_j) / (1 - 2 tau_j) every later round of the claims under that eq has l(1) p = 0: the reference takes the
    fallback in all of them, and their parts of every later round polynomial vanish"""
    p = fc.FIELDS[fid]
    l = 5
    rng = random.Random(91 + fid)
    rho, ro = [rng.randrange(p) for _ in range(l)], [rng.randrange(p) for _ in range(l)]
    for j in (0, 2, l - 1):
        both(fid, l, seed=500 + j, rhos=rho, r_outer=ro, force={j: pc.zeroing_challenge(p, rho[j])})
        both(fid, l, seed=510 + j, rhos=rho, r_outer=ro, force={j: pc.zeroing_challenge(p, ro[j])})


def test_every_entry_and_scalar_p_minus_one():
    for fid in (0, 1, 2, 3):
        for l in (1, 5):
            both(fid, l, seed=62, fill=fc.FIELDS[fid] - 1)


def test_standalone_program_of_the_host_tail():
    """the same source with its own main(): the form a sanitizer build of the host tail takes (g++ -fsanitize=address,undefined -DSCP_MAIN)"""
    src = os.path.join(ROOT, "tests", "cpp", "sc_ppsnark_host_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "sc_ppsnark_host_test.bin")
    deps = [src] + [os.path.join(CSRC, f) for f in ("sc_host.hpp", "host_fp4.hpp", "fp.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DSCP_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "sc_ppsnark host tail ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


# ---- (3) the kernels' lane bodies under the emulation ------------------------------------------------------------------------------
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "sc_ppsnark_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_sc_ppsnark_emul.so")
RI = 1 << 261          # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)
BIG = 2 * 256 + 1      # two blocks' worth of indices and one more: a partial last block, more than one block
MEM, INNER, WIT, ALL = 0, 2, 4, 6
NTAB, NSUM = {MEM: 5, INNER: 4, WIT: 2, ALL: 16}, {MEM: 6, INNER: 4, WIT: 2}


@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in ("fp.hpp", "sumcheck_ppsnark.hpp", "sumcheck_inplace.hpp", "spmv_row.hpp",
                                                                                                            "msm_partition.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.emul_sc_ppsnark.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, vp, u32, vp]
    return lib


def words(vals):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals), np.uint32).copy()


class Inst:
    """one group's tables of `length` stored (canonical) elements and eq tables of both forms for `nidx` indices"""

    def __init__(self, fid, group, length, nidx, seed, first_half, fill=None):
        self.fid, self.group, self.p = fid, group, fc.FIELDS[fid]
        p, rng = self.p, random.Random(seed)
        val = (lambda: fill) if fill is not None else (lambda: rng.choice([0, 1, p - 1, p - 2]) if rng.random() < 0.1 else rng.randrange(p))
        self.T = [[val() for _ in range(length)] for _ in range(NTAB[group])]
        self.shift = 5 if first_half else 0
        if first_half:
            self.eqR, self.eqL = [val() for _ in range(32)], [val() for _ in range((nidx + 31) // 32)]
            self.fac = [self.eqL[i >> 5] * self.eqR[i & 31] % p for i in range(nidx)]
            self.neq = 2                                      # device products behind the eq factor
        else:
            self.eqR, self.eqL = [val() for _ in range(max(nidx, 1))], None
            self.fac = list(self.eqR)
            self.neq = 1

    def run(self, E, bind_pass, n, with_inf=1, bind=0, r=None, grid=None, offset=0):
        """-> the group's sums over the lanes, mod p; the tables are updated in place by the bind passes; self.stage: the staging area"""
        p, g = self.p, self.group
        bufs = [words(t) for t in self.T]
        ptrs = (ctypes.c_void_p * len(bufs))(*[b.ctypes.data + 32 * offset for b in bufs])
        nk, one = words([p - 1]), words([1])
        rw = words([r * RI % p]) if r is not None else None
        eqL, eqR = (words(self.eqL) if self.eqL else None), words(self.eqR)
        grid = grid or max(1, (n + 255) // 256)
        stage = np.full(16 * max(n, 1) * 8, 0xdeadbeef, np.uint32)
        J = NSUM.get(g, 1)
        lanes = np.zeros(grid * 256 * J * 8, np.uint32)
        rc = E.emul_sc_ppsnark(self.fid, g + (1 if bind_pass else 0) if g != ALL else ALL, ctypes.addressof(ptrs), nk.ctypes.data, one.ctypes.data,
                               rw.ctypes.data if r is not None else None, eqL.ctypes.data if eqL is not None else None, eqR.ctypes.data, self.shift, n,
                               with_inf, bind, stage.ctypes.data, grid, lanes.ctypes.data)
        assert rc == 0
        self.T = [fc.ints(b.view(np.uint8)) for b in bufs]
        self.stage = fc.ints(stage.view(np.uint8))
        sums = fc.ints(lanes.view(np.uint8))
        assert all(s < p for s in sums), "a lane's sum is not the canonical representative"
        return [sum(sums[j::J]) % p for j in range(J)]

    def want(self, n, T=None, base=0, with_inf=True):
        """the group's sums over indices [0, n) of tables read at base + id and base + n + id, scaled as the device leaves them"""
        p, T, g, f = self.p, T or self.T, self.group, self.fac
        lo, hi = (lambda X, i: X[base + i]), (lambda X, i: X[base + n + i])
        d, m1 = (lambda X, i: hi(X, i) - lo(X, i)), (lambda X, i: 2 * lo(X, i) - hi(X, i))
        s = lambda k: pow(RI, -k, p)  # noqa: E731
        R = range(n)
        if g == MEM:
            t, tinv, w, winv, ts = T
            out = [0, 0, sum((lo(tinv, i) * lo(t, i) - lo(ts, i)) * f[i] for i in R) * s(1 + self.neq), 0,
                   sum((lo(winv, i) * lo(w, i) - 1) * f[i] for i in R) * s(1 + self.neq), 0]
            if with_inf:
                out[0], out[1] = sum(lo(tinv, i) - lo(winv, i) for i in R), sum(hi(tinv, i) - hi(winv, i) for i in R)
                out[3] = sum(d(tinv, i) * d(t, i) * f[i] for i in R) * s(1 + self.neq)
                out[5] = sum(d(winv, i) * d(w, i) * f[i] for i in R) * s(1 + self.neq)
        elif g == INNER:
            a, b, c, e = T
            out = [0, 0, 0, sum(lo(e, i) * f[i] for i in R) * s(self.neq)]
            if with_inf:
                out[0] = sum(lo(a, i) * lo(b, i) * lo(c, i) for i in R) * s(2)
                out[1] = sum(d(a, i) * d(b, i) * d(c, i) for i in R) * s(2)
                out[2] = sum(m1(a, i) * m1(b, i) * m1(c, i) for i in R) * s(2)
        else:
            a, b = T
            out = [sum(lo(a, i) * lo(b, i) for i in R) * s(1), sum(m1(a, i) * m1(b, i) for i in R) * s(1)]
        return [x % p for x in out]


@pytest.mark.parametrize("first_half", [True, False])
@pytest.mark.parametrize("group", [MEM, INNER, WIT])
@pytest.mark.parametrize("n", [1, BIG])
def test_emulated_sums_pass(E, n, group, first_half):
    for fid in ((0, 1, 2, 3) if n == 1 else (1, 2)):
        x = Inst(fid, group, 2 * n, n, seed=7 * group + n, first_half=first_half)
        assert x.run(E, False, n) == x.want(n)
        assert x.run(E, False, n, grid=1) == x.want(n)                  # one block: every lane walks several indices
        if group != WIT:    # the fallback's t(1): the same pass pointed at the high halves, the t(0) sums alone -- nothing is read beyond the tables
            assert x.run(E, False, n, with_inf=0, offset=n) == x.want(n, base=n, with_inf=False)


@pytest.mark.parametrize("first_half", [True, False])
@pytest.mark.parametrize("group", [MEM, INNER, WIT])
@pytest.mark.parametrize("hq", [1, BIG])
def test_emulated_bind_and_sums_pass(E, hq, group, first_half):
    for fid in ((0, 1, 2, 3) if hq == 1 else (1, 3)):
        x = Inst(fid, group, 4 * hq, hq, seed=11 * group + hq, first_half=first_half)
        p, r = x.p, random.Random(hq + group).randrange(x.p)
        bound = [[(t[i] + r * (t[i + 2 * hq] - t[i])) % p for i in range(2 * hq)] for t in x.T]
        old = x.T
        got = x.run(E, True, hq, r=r)
        assert [t[:2 * hq] for t in x.T] == bound, "the stored halves are lo + r (hi - lo)"
        assert [t[2 * hq:] for t in x.T] == [t[2 * hq:] for t in old], "the high halves are not written"
        assert got == x.want(hq, T=bound)


@pytest.mark.parametrize("half", [1, BIG])
def test_emulated_last_bind_without_sums(E, half):
    for fid in (1, 2):
        x = Inst(fid, ALL, 2 * half, half, seed=half, first_half=False)
        p, r = x.p, random.Random(half).randrange(x.p)
        bound = [[(t[i] + r * (t[i + half] - t[i])) % p for i in range(half)] for t in x.T]
        x.run(E, False, half, bind=1, r=r)
        assert [t[:half] for t in x.T] == bound
        assert x.stage == [v for t in bound for v in t], "the staging area holds the sixteen bound tables contiguously, in table order"
        before = x.T
        x.run(E, False, half, bind=0)                                   # no bind: the tables as they are, untouched
        assert x.T == before and x.stage == [v for t in before for v in t[:half]]


@pytest.mark.parametrize("first_half", [True, False])
@pytest.mark.parametrize("group", [MEM, INNER, WIT])
def test_emulated_passes_with_every_entry_p_minus_one(E, group, first_half):
    """the lazy accumulators' limb and value bounds (sumcheck_ppsnark.hpp kScPpsLazy) at their worst: everything p - 1, a lane walking
    several indices; then operands that make every difference large with mixed signs"""
    for fid in (0, 1, 2, 3):
        p = fc.FIELDS[fid]
        x = Inst(fid, group, 2 * 600, 600, seed=1, first_half=first_half, fill=p - 1)
        assert x.run(E, False, 600, grid=1) == x.want(600)
        x = Inst(fid, group, 4 * 300, 300, seed=1, first_half=first_half, fill=p - 1)
        bound = [[p - 1] * 600 for _ in x.T]                            # lo + r (hi - lo) with hi == lo
        assert x.run(E, True, 300, r=p - 1, grid=1) == x.want(300, T=bound)
        y = Inst(fid, group, 2 * 64, 64, seed=2, first_half=first_half, fill=p - 1)
        y.T = [[(p - 1) if (i >= 64) ^ ((t + i) % 2 == 0) else 0 for i in range(128)] for t in range(NTAB[group])]   # low 0 / high p - 1 and back
        assert y.run(E, False, 64) == y.want(64)
        assert y.run(E, False, 64, grid=1) == y.want(64)
