"""nmx_sumcheck_prove_batched_cubic without a GPU.  (1) The entry point is declared, exported and bound in Python / C++ / Rust, and its
argument errors return with no device present.  (2) The host tail (sc_tail_rounds_batched, nova_amd/csrc/sc_host.hpp) compiled with g++
as a complete prover over host tables (tests/cpp/sc_batched_host_test.cpp) passes check_batched_cubic -- the reference's verifier, the
final evaluations, the definition of every round polynomial -- and equals the plain restatement of the reference in Python integers
(tests/batched_cubic_common.py_prove) output for output, the tau = 0 fallback and the eq-zeroing challenge included.  (3) The lane
bodies of the two new kernels and of the sum-less last bind (nova_amd/csrc/sumcheck_batched.hpp) run thread by thread under
tests/host_emul/simt.hpp with limb bounds asserted, against big-integer sums.  What the emulation does NOT run: the block reduction
(shuffles), k_sum_partials_mail and the host half of the device rounds; tests/test_gpu_sumcheck_batched.py covers those."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import cref
from tests import batched_cubic_common as bc
from tests import fv_common as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
PARAMS = ["int field_id", "const void* claim", "const void* taus", "size_t num_rounds", "void* const* As", "void* const* Bs", "void* const* Cs",
          "const void* alphas", "size_t k", "uint32_t flags", "nmx_transcript_fn transcript", "void* ctx", "uint8_t* out_polys", "uint8_t* out_r",
          "uint8_t* out_claims"]


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
    m = re.search(r"int nmx_sumcheck_prove_batched_cubic\(([^;]*)\);", hdr)
    assert m, "the header does not declare nmx_sumcheck_prove_batched_cubic"
    assert [x.strip() for x in re.sub(r"\s+", " ", m.group(1)).split(",")] == PARAMS
    assert hasattr(L, "nmx_sumcheck_prove_batched_cubic")
    ctype_of = lambda d: (ctypes.c_int if d.startswith("int ") else ctypes.c_size_t if d.startswith("size_t") else ctypes.c_uint32  # noqa: E731
                          if d.startswith("uint32_t") else _lib.TRANSCRIPT_FN if d.startswith("nmx_transcript_fn") else ctypes.c_void_p)
    assert list(L.nmx_sumcheck_prove_batched_cubic.argtypes) == [ctype_of(d) for d in PARAMS]
    doc = hdr.split("int nmx_sumcheck_prove_batched_cubic(")[0].rsplit("/*", 1)[1]
    for needle in ("sumcheck.rs:509-577", "sumcheck.rs:749-894", "1 <= k <= 16", "NMX_E_ARG", "NMX_E_SCALAR_RANGE", "BOUND IN PLACE", "overlapping",
                   "sc_host_tail", "sc_poll_us", "do NOT affect"):
        assert needle in doc, needle
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    assert "pub fn nmx_sumcheck_prove_batched_cubic(" in ffi, "ffi.rs: regenerate with scripts/gen_rust_sys.py"


def test_python_and_cpp_wrappers_exist():
    import inspect
    from nova_amd import fieldvec as fv
    assert list(inspect.signature(fv.sumcheck_prove_batched_cubic).parameters) == ["field", "claim", "taus", "As", "Bs", "Cs", "alphas", "transcript",
                                                                                   "mont", "ctx"]
    hpp = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read()
    assert "static SumcheckProof prove_batched_cubic(const Scalar& claim" in hpp
    assert "inline Proof prove_batched_cubic(int field" in hpp.split("namespace resident {")[1]
    z, cb = fc.vec([0, 0]), (lambda c: bytes(32))
    for nb, nc, na in ((1, 2, 2), (2, 3, 2), (2, 2, 3)):      # the reference's assert_eq!(k, ...) lines (sumcheck.rs:526-528)
        with pytest.raises(AssertionError, match="assert_eq"):
            fv.sumcheck_prove_batched_cubic(1, bytes(32), fc.vec([1]), [z] * 2, [z] * nb, [z] * nc, fc.vec([1] * na), cb)


def test_argument_errors_need_no_device_and_touch_nothing(L):
    from nova_amd import _lib
    fid, l = 1, 3
    p = fc.FIELDS[fid]
    cb = _lib.TRANSCRIPT_FN(lambda *_a: 1)
    big = np.ascontiguousarray(fc.rand_vec(fid, 6 * (1 << l) + 4, 3).copy())
    before = big.copy()
    tab = lambda i, off=0: big.ctypes.data + 32 * ((1 << l) * i + off)  # noqa: E731

    def call(k=2, A=None, B=None, C=None, claim=1, taus=(2, 3, 4), alphas=(5, 6), field=fid, cb_=cb, nr=l):
        arr = lambda v: (ctypes.c_void_p * 17)(*v)  # noqa: E731
        A, B, C = A or [tab(0), tab(1)] + [tab(0)] * 15, B or [tab(2), tab(3)] + [tab(0)] * 15, C or [tab(4), tab(5)] + [tab(0)] * 15
        cl, tv, av = fc.vec([claim]).copy(), fc.vec(list(taus)).copy(), fc.vec(list(alphas) + [1] * 16).copy()
        return L.nmx_sumcheck_prove_batched_cubic(field, cl.ctypes.data, tv.ctypes.data, nr, arr(A), arr(B), arr(C), av.ctypes.data, k, 0, cb_, None,
                                                  None, None, None)
    assert call(k=0) == _lib.E_ARG                                    # the reference's InvalidNumInstances
    assert b"between 1 and 16" in L.nmx_last_error()
    assert call(k=17) == _lib.E_ARG
    assert call(B=[tab(2), None] + [tab(0)] * 15) == _lib.E_ARG       # a NULL table
    assert call(B=[tab(2), tab(0)] + [tab(0)] * 15) == _lib.E_ARG     # Bs[1] aliases As[0]
    assert b"overlap" in L.nmx_last_error()
    assert call(C=[tab(4), tab(4, 4)] + [tab(0)] * 15) == _lib.E_ARG  # a table overlapping another by half
    assert call(alphas=(5, p)) == _lib.E_SCALAR_RANGE
    assert call(taus=(2, p + 1, 4)) == _lib.E_SCALAR_RANGE
    assert call(claim=p) == _lib.E_SCALAR_RANGE
    assert call(field=4) == _lib.E_ARG and call(field=-1) == _lib.E_ARG
    assert call(cb_=_lib.TRANSCRIPT_FN()) == _lib.E_ARG               # null callback
    assert call(nr=31) != 0
    assert (big == before).all()


# ---- (2) the host prover ------------------------------------------------------------------------------------------------------------
_hlib = None


def hscb():
    global _hlib
    if _hlib is None:
        so = os.path.join(ROOT, "tests", "cpp", "libsc_batched_host_test.so")
        src = os.path.join(ROOT, "tests", "cpp", "sc_batched_host_test.cpp")
        deps = [src] + [os.path.join(CSRC, f) for f in ("sc_host.hpp", "host_fp4.hpp", "fp.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
        _hlib = ctypes.CDLL(so)
    return _hlib


def h_prove(fid, claim, taus, As, Bs, Cs, alphas, tr, mont=0):
    k = len(As)
    keep = [np.ascontiguousarray(x) for x in list(As) + list(Bs) + list(Cs)]
    ptrs = [(ctypes.c_void_p * k)(*[a.ctypes.data for a in keep[w * k:(w + 1) * k]]) for w in range(3)]
    cl = np.frombuffer(bytes(claim), np.uint8).copy()
    tv, av = np.ascontiguousarray(taus), np.ascontiguousarray(alphas)
    nr = tv.size // 32
    polys, r, out = np.zeros(128 * max(nr, 1), np.uint8), np.zeros(32 * max(nr, 1), np.uint8), np.zeros(96 * k, np.uint8)
    cb = cref.make_transcript(tr)
    vp = ctypes.c_void_p
    rc = hscb().hscb_prove_batched_cubic(fid, mont, vp(cl.ctypes.data), vp(tv.ctypes.data), ctypes.c_size_t(nr), ptrs[0], ptrs[1], ptrs[2],
                                         vp(av.ctypes.data), ctypes.c_size_t(k), cb, None, vp(polys.ctypes.data), vp(r.ctypes.data), vp(out.ctypes.data))
    assert rc == 0
    pb, rb, ob = polys.tobytes(), r.tobytes(), out.tobytes()
    return ([[pb[128 * j + 32 * i: 128 * j + 32 * i + 32] for i in range(4)] for j in range(nr)], [rb[32 * j: 32 * j + 32] for j in range(nr)],
            [[ob[96 * i + 32 * w: 96 * i + 32 * w + 32] for w in range(3)] for i in range(k)])


def both(fid, l, k, **kw):
    got = bc.check_batched_cubic(h_prove, fid, l, k, **kw)
    assert got == bc.check_batched_cubic(bc.py_prove, fid, l, k, **kw), "the host prover and the restatement of the reference disagree"
    return got


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("l", [1, 2, 3, 5, 8])
def test_host_prover(fid, l):
    for k in (1, 2, 3, 16):
        both(fid, l, k, seed=1000 + 10 * l + k)


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("l", [1, 2, 3, 5, 8])
def test_host_prover_montgomery_words(fid, l):
    for k in (1, 2, 3, 16):
        prove_m = bc.montgomery_wrapped(lambda *a: h_prove(*a, mont=1), fid)
        assert bc.check_batched_cubic(prove_m, fid, l, k, seed=50 + l) == bc.check_batched_cubic(bc.py_prove, fid, l, k, seed=50 + l)


@pytest.mark.parametrize("fid", [1, 2])
@pytest.mark.parametrize("l", [1, 4, 7])
def test_one_triple_with_alpha_one_is_the_cubic_prover_byte_for_byte(fid, l):
    from tests import test_sc_host as tsh
    from tests import spartan_common as sp
    As, Bs, Cs, tv, _av = bc.make_instance(fid, l, 1, seed=33)
    p = fc.FIELDS[fid]
    eqt = bc.eq_table(p, fc.ints(tv))
    claim = sp.le(sum(e * (a * b - c) for e, a, b, c in zip(eqt, fc.ints(As[0]), fc.ints(Bs[0]), fc.ints(Cs[0]))) % p)
    t1, t2 = sp.StandInTranscript(p), sp.StandInTranscript(p)
    polys, rs, claims = h_prove(fid, claim, tv, As, Bs, Cs, fc.vec([1]), t1)
    polys3, rs3, claims3 = tsh.h_cubic3(fid, claim, tv, As[0], Bs[0], Cs[0], t2)
    assert (polys, rs, claims[0]) == (polys3, rs3, claims3)


@pytest.mark.parametrize("l", [3, 6])
def test_fallback_when_a_tau_is_zero(l):
    fid = 1
    base = fc.ints(fc.rand_vec(fid, l, 55))
    for zero_at in (0, l // 2, l - 1):      # the first round, a middle round, the last round (sumcheck.rs:839-894)
        taus = list(base)
        taus[zero_at] = 0
        for force in (None, {zero_at: 1}):
            both(fid, l, 3, seed=400 + zero_at, taus=taus, force=force)
    both(fid, l, 2, seed=77, taus=[0] * l)


@pytest.mark.parametrize("fid", [1, 3])
def test_a_challenge_that_zeroes_the_running_eq_product(fid):
    """after r_j = (1 - tau_j) / (1 - 2 tau_j) every later round has l(1) p = 0: the reference takes the fallback in all of them"""
    p = fc.FIELDS[fid]
    l = 5
    taus = fc.ints(fc.rand_vec(fid, l, 91))
    for j in (0, 2, l - 1):
        polys, _rs, _cl = both(fid, l, 3, seed=500 + j, taus=taus, force={j: bc.zeroing_challenge(p, taus[j])})
        assert all(c == bytes(32) for row in polys[j + 1:] for c in row), "every later round polynomial is zero"


def test_an_alpha_of_zero_and_all_entries_p_minus_one():
    for fid in (0, 1, 2, 3):
        p = fc.FIELDS[fid]
        al = fc.ints(fc.rand_vec(fid, 3, 5))
        al[1] = 0
        both(fid, 4, 3, seed=61, alphas=al)
        both(fid, 5, 16, seed=62, alphas=[p - 1] * 16, fill=p - 1)


def test_standalone_program_of_the_host_tail():
    """the same source with its own main(): the form a sanitizer build of the host tail takes (g++ -fsanitize=address,undefined -DSCB_MAIN)"""
    src = os.path.join(ROOT, "tests", "cpp", "sc_batched_host_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "sc_batched_host_test.bin")
    deps = [src] + [os.path.join(CSRC, f) for f in ("sc_host.hpp", "host_fp4.hpp", "fp.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DSCB_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "sc_batched host tail ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


# ---- (3) the kernels' lane bodies under the emulation ------------------------------------------------------------------------------
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "sc_batched_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_sc_batched_emul.so")
RI = 1 << 261          # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)
BIG = 3 * 256 + 1      # three blocks' worth of indices and one more: a partial last block, more than one block


@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in ("fp.hpp", "sumcheck_batched.hpp", "sumcheck_inplace.hpp", "spmv_row.hpp",
                                                                                                            "msm_partition.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.emul_sc_batched.argtypes = [ctypes.c_int, ctypes.c_int, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, vp, u32, vp]
    return lib


def words(vals):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals), np.uint32).copy()


class Inst:
    """k triples of `length` stored (canonical) elements, alphas, eq tables of both forms for `nidx` indices"""

    def __init__(self, fid, k, length, nidx, seed, first_half, fill=None):
        self.fid, self.k, self.p = fid, k, fc.FIELDS[fid]
        p, rng = self.p, random.Random(seed)
        val = (lambda: fill) if fill is not None else (lambda: rng.choice([0, 1, p - 1, p - 2]) if rng.random() < 0.1 else rng.randrange(p))
        self.T = [[[val() for _ in range(length)] for _ in range(k)] for _ in range(3)]       # [A, B, C][i][x]
        self.al = [val() for _ in range(k)]
        self.shift = 5 if first_half else 0
        if first_half:
            self.eqR, self.eqL = [val() for _ in range(32)], [val() for _ in range((nidx + 31) // 32)]
            self.fac = [self.eqL[i >> 5] * self.eqR[i & 31] % p for i in range(nidx)]
            self.nfac = 3                                     # device products behind a term: alpha-sum x (eqL x eqR): R'^-3 in all
        else:
            self.eqR, self.eqL = [val() for _ in range(nidx)], None
            self.fac = list(self.eqR)
            self.nfac = 2

    def run(self, E, which, n, with_inf=1, bind=0, r=None, grid=None, offset=0):
        """-> (s0, s1) summed over the lanes, mod p; the tables are updated in place by the bind passes; self.stage: the staging area"""
        p, k = self.p, self.k
        bufs = [[words(t) for t in tabs] for tabs in self.T]
        arr = lambda bs: (ctypes.c_void_p * k)(*[b.ctypes.data + 32 * offset for b in bs])  # noqa: E731
        al, nk = words([a * RI % p for a in self.al]), words([p - 1])
        rw = words([r * RI % p]) if r is not None else None
        eqL, eqR = (words(self.eqL) if self.eqL else None), words(self.eqR)
        grid = grid or max(1, (n + 255) // 256)
        stage = np.full(3 * k * max(n, 1) * 8, 0xdeadbeef, np.uint32)
        lanes = np.zeros(grid * 256 * 16, np.uint32)
        ptrs = [arr(b) for b in bufs]
        rc = E.emul_sc_batched(self.fid, which, k, *[ctypes.addressof(x) for x in ptrs], al.ctypes.data, nk.ctypes.data, rw.ctypes.data if r is not None else None,
                               eqL.ctypes.data if eqL is not None else None, eqR.ctypes.data, self.shift, n, with_inf, bind, stage.ctypes.data, grid,
                               lanes.ctypes.data)
        assert rc == 0
        self.T = [[fc.ints(b.view(np.uint8)) for b in bs] for bs in bufs]
        self.stage = fc.ints(stage.view(np.uint8))
        sums = fc.ints(lanes.view(np.uint8))
        assert all(s < p for s in sums), "a lane's sum is not the canonical representative"
        return sum(sums[0::2]) % p, sum(sums[1::2]) % p

    def want(self, n, T=None, base=0, with_inf=True):
        """the two sums over indices [0, n) of tables read at base + id and base + n + id, scaled as the device leaves them"""
        p, T = self.p, T or self.T
        A, B, C = T
        s0 = s1 = 0
        for i in range(n):
            e = sum(al * (a[base + i] * b[base + i] - c[base + i]) for al, a, b, c in zip(self.al, A, B, C))
            s0 += e * self.fac[i]
            if with_inf:
                q = sum(al * (a[base + n + i] - a[base + i]) * (b[base + n + i] - b[base + i]) for al, a, b in zip(self.al, A, B))
                s1 += q * self.fac[i]
        scale = pow(RI, -self.nfac, p)
        return s0 * scale % p, s1 * scale % p


@pytest.mark.parametrize("first_half", [True, False])
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("n", [1, BIG])
def test_emulated_sums_pass(E, n, k, first_half):
    for fid in ((0, 1, 2, 3) if n == 1 else (1, 2)):
        x = Inst(fid, k, 2 * n, n, seed=7 * k + n, first_half=first_half)
        assert x.run(E, 0, n) == x.want(n)
        assert x.run(E, 0, n, grid=1) == x.want(n)                    # one block: every lane walks several indices
        # the fallback's t(1): the same pass pointed at the high halves, t(0)'s sum alone -- nothing is read beyond the tables
        assert x.run(E, 0, n, with_inf=0, offset=n) == x.want(n, base=n, with_inf=False)


@pytest.mark.parametrize("first_half", [True, False])
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("hq", [1, BIG])
def test_emulated_bind_and_sums_pass(E, hq, k, first_half):
    for fid in ((0, 1, 2, 3) if hq == 1 else (1, 3)):
        x = Inst(fid, k, 4 * hq, hq, seed=11 * k + hq, first_half=first_half)
        p, r = x.p, random.Random(hq + k).randrange(x.p)
        bound = [[[(t[i] + r * (t[i + 2 * hq] - t[i])) % p for i in range(2 * hq)] for t in tabs] for tabs in x.T]
        old = x.T
        got = x.run(E, 1, hq, r=r)
        assert [[t[:2 * hq] for t in tabs] for tabs in x.T] == bound, "the stored halves are lo + r (hi - lo)"
        assert [[t[2 * hq:] for t in tabs] for tabs in x.T] == [[t[2 * hq:] for t in tabs] for tabs in old], "the high halves are not written"
        assert got == x.want(hq, T=bound)


@pytest.mark.parametrize("half", [1, BIG])
def test_emulated_last_bind_without_sums(E, half):
    for fid, k in ((1, 1), (2, 3), (3, 16)):
        x = Inst(fid, k, 2 * half, half, seed=half + k, first_half=False)
        p, r = x.p, random.Random(half).randrange(x.p)
        bound = [[[(t[i] + r * (t[i + half] - t[i])) % p for i in range(half)] for t in tabs] for tabs in x.T]
        x.run(E, 2, half, bind=1, r=r)
        assert [[t[:half] for t in tabs] for tabs in x.T] == bound
        assert x.stage == [v for i in range(k) for w in range(3) for v in bound[w][i]], "the staging area holds A_0, B_0, C_0, A_1, ... contiguously"
        before = x.T
        x.run(E, 2, half, bind=0)                                        # no bind: the tables as they are, untouched
        assert x.T == before and x.stage == [v for i in range(k) for w in range(3) for v in before[w][i][:half]]


@pytest.mark.parametrize("first_half", [True, False])
def test_emulated_passes_with_every_entry_and_alpha_p_minus_one(E, first_half):
    """the lazy accumulators' limb and value bounds (sumcheck_batched.hpp ScBatchedAcc) at their worst: 16 triples, everything p - 1"""
    for fid in (0, 1, 2, 3):
        p = fc.FIELDS[fid]
        x = Inst(fid, 16, 4 * 300, 600, seed=1, first_half=first_half, fill=p - 1)
        assert x.run(E, 0, 600, grid=1) == x.want(600)
        x = Inst(fid, 16, 4 * 300, 300, seed=1, first_half=first_half, fill=p - 1)
        bound = [[[p - 1] * 600 for _ in tabs] for tabs in x.T]       # lo + r (hi - lo) with hi == lo
        assert x.run(E, 1, 300, r=p - 1, grid=1) == x.want(300, T=bound)
        # and operands that make every product large with mixed signs: alternate 1 and p - 1
        y = Inst(fid, 16, 2 * 64, 64, seed=2, first_half=first_half, fill=p - 1)
        y.T = [[[(p - 1) if (i + w + j) % 2 else 1 for j in range(128)] for i in range(16)] for w in range(3)]
        assert y.run(E, 0, 64) == y.want(64)
