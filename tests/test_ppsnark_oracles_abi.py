"""nmx_field_gather / nmx_ppsnark_mem_oracles without a GPU.  (1) Both entry points are declared with the header's parameter lists,
exported, bound in Python / C++ / Rust, and the header names the reference's line ranges and every error code.  (2) Every argument error
of the header returns its code with no device present and leaves the caller's buffers byte-identical.  (3) The lane bodies of the kernels
(nova_amd/csrc/ppsnark_oracles.hpp) run thread by thread under tests/host_emul/simt.hpp with limb bounds asserted, against the definition in
Python integers (tests/ppsnark_oracles_common.py) on all four fields, canonical and Montgomery words: the gather with its refusals, and both
level-0 passes of the oracles with the kernels' own chunk -> (segment, local chunk) map, the chunk products inverted HERE in between.
What the emulation does NOT run: the launches, the staging, the levels above level 0 and the host top (nmx_field_batch_invert's code);
tests/test_gpu_ppsnark_oracles.py covers those."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fv_common as fc
from tests import ppsnark_oracles_common as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
G_PARAMS = ["int field_id", "const void* mem", "size_t n_mem", "const void* addr", "size_t n", "uint32_t flags", "void* out"]
O_PARAMS = ["int field_id", "size_t k", "size_t n", "const void* const* mem", "const void* const* addr", "const void* const* L", "const void* const* ts",
            "const void* gamma", "const void* r", "uint32_t flags", "void* const* out_t_plus_r", "void* const* out_w_plus_r",
            "void* const* out_t_plus_r_inv", "void* const* out_w_plus_r_inv"]


@pytest.fixture(scope="module")
def L():
    from nova_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- (1) the surface ----------------------------------------------------------------------------------------------------------------
def test_header_declares_library_exports_and_python_binds_the_same_types(L):
    hdr = open(os.path.join(ROOT, "include", "nova_mi355x.h")).read()
    ctype_of = lambda d: (ctypes.c_int if d.startswith("int ") else ctypes.c_size_t if d.startswith("size_t") else ctypes.c_uint32  # noqa: E731
                          if d.startswith("uint32_t") else ctypes.c_void_p)
    for name, want in (("nmx_field_gather", G_PARAMS), ("nmx_ppsnark_mem_oracles", O_PARAMS)):
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, "the header does not declare " + name
        plist = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert [x.strip() for x in re.sub(r"\s+", " ", plist).split(",")] == want
        assert hasattr(L, name)
        assert list(getattr(L, name).argtypes) == [ctype_of(d) for d in want]
    assert hdr.index("int nmx_sumcheck_prove_ppsnark(") < hdr.index("int nmx_field_gather(") < hdr.index("int nmx_ppsnark_mem_oracles(")
    g_doc = hdr.split("int nmx_field_gather(")[0].rsplit("/* ---- ppsnark's lookup gather", 1)[1]
    for needle in ("ppsnark.rs:220-253", "ppsnark.rs:180-181", "NMX_E_ARG", "NMX_E_TOO_LARGE", "NMX_SCALARS_MONT", "NMX_SCALARS_DEVICE", "NMX_ASYNC", "unspecified",
                   "n == 0", "nothing written", "overlapping"):
        assert needle in g_doc, needle
    o_doc = hdr.split("int nmx_ppsnark_mem_oracles(")[0].rsplit("/* nmx_ppsnark_mem_oracles ==", 1)[1]
    for needle in ("ppsnark.rs:371-489", "ppsnark.rs:430", "NMX_E_ZERO", "NMX_E_ARG", "NMX_E_SCALAR_RANGE", "NMX_E_TOO_LARGE", "NMX_ASYNC", "unspecified",
                   "NMX_PPS_T_ROW + 5 m", "NMX_PPS_W_ROW + 5 m", "NMX_PPS_TINV_ROW + 5 m", "NMX_PPS_WINV_ROW + 5 m", "nothing written", "canonical"):
        assert needle in o_doc, needle
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    assert "pub fn nmx_field_gather(" in ffi and "pub fn nmx_ppsnark_mem_oracles(" in ffi, "ffi.rs: regenerate with scripts/gen_rust_sys.py"


def test_python_and_cpp_wrappers_exist():
    from nova_amd import fieldvec as fv
    assert list(inspect.signature(fv.gather).parameters) == ["field", "mem", "addr", "mont"]
    assert list(inspect.signature(fv.ppsnark_mem_oracles).parameters) == ["field", "mems", "addrs", "Ls", "tss", "gamma", "r", "mont"]
    res = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read().split("namespace resident {")[1]
    for decl in ("inline void gather(int field", "inline void ppsnark_mem_oracles(int field"):
        assert decl in res, decl
    assert '#include "ppsnark_oracles.hpp"' in open(os.path.join(CSRC, "fieldvec.hip")).read()


# ---- (2) argument errors --------------------------------------------------------------------------------------------------------------
def test_gather_argument_errors_need_no_device_and_touch_nothing(L):
    from nova_amd import _lib
    fid = 1
    buf = np.ascontiguousarray(fc.rand_vec(fid, 64, 3).copy())      # mem = [0, 10), addr = [16, 24), out = [32, 40)
    before = buf.copy()
    at = lambda i: buf.ctypes.data + 32 * i  # noqa: E731

    def g(field=fid, mem=at(0), n_mem=10, addr=at(16), n=8, flags=0, out=at(32)):
        return L.nmx_field_gather(field, mem, n_mem, addr, n, flags, out)
    A, TL = _lib.E_ARG, _lib.E_TOO_LARGE
    assert g(mem=None) == A and g(addr=None) == A and g(out=None) == A
    assert g(n_mem=0) == A
    assert g(field=4) == A and g(field=-1) == A
    assert b"bad field id" in L.nmx_last_error()
    for fl in (_lib.ASYNC, _lib.BASES_MONT, _lib.BASES_DEVICE, _lib.OUT_PARTIAL, 1 << 20, _lib.ASYNC | _lib.SCALARS_DEVICE):
        assert g(flags=fl) == A, fl
    assert g(n=1 << 32) == TL and g(n_mem=1 << 32) == TL and g(n=(1 << 63) + 1) == TL
    # out over mem or addr, by one element at either end
    assert g(out=at(9)) == A and g(out=at(0)) == A and g(mem=at(39)) == A
    assert b"overlap" in L.nmx_last_error()
    assert g(out=at(23)) == A and g(out=at(16)) == A and g(out=at(9), n=8) == A and g(addr=at(39)) == A
    assert (buf == before).all(), "a refused call wrote something"
    # n == 0 is NMX_OK with no launch -- and so needs no device; a well-formed call gets past every check
    assert g(n=0) == 0 and g(n=0, n_mem=0) == 0
    ok = 0 if L.nmx_device_count() > 0 else _lib.E_NO_DEVICE
    buf[16:24] = fc.vec([0, 9, 1, 2, 3, 9, 0, 5])
    before = buf.copy()
    assert g() == ok and g(flags=_lib.SCALARS_MONT) in (ok, A)       # (Montgomery words of small integers are addresses far beyond n_mem)
    if ok:
        assert (buf == before).all()


def test_oracle_argument_errors_need_no_device_and_touch_nothing(L):
    from nova_amd import _lib
    fid, n = 1, 4
    p = fc.FIELDS[fid]
    buf = np.ascontiguousarray(fc.rand_vec(fid, 32 * n, 5).copy())  # vector j of 16 = [n j, n j + n): 8 inputs, then 8 outputs
    before = buf.copy()
    at = lambda j, off=0: buf.ctypes.data + 32 * (n * j + off)  # noqa: E731
    good = {"mem": [at(0), at(1)], "addr": [at(2), at(3)], "L": [at(4), at(5)], "ts": [at(6), at(7)],
            "t": [at(8), at(9)], "w": [at(10), at(11)], "tinv": [at(12), at(13)], "winv": [at(14), at(15)]}
    names = ["mem", "addr", "L", "ts", "t", "w", "tinv", "winv"]

    def o(field=fid, k=2, n_=n, gamma=3, r=5, flags=0, null=None, **over):
        v = dict(good, **over)
        arr = {nm: (None if v[nm] is None else (ctypes.c_void_p * 8)(*(list(v[nm]) + [None] * (8 - len(v[nm]))))) for nm in names}
        gw, rw = fc.vec([gamma]).copy(), fc.vec([r]).copy()
        return L.nmx_ppsnark_mem_oracles(field, k, n_, arr["mem"], arr["addr"], arr["L"], arr["ts"], None if null == "gamma" else gw.ctypes.data,
                                         None if null == "r" else rw.ctypes.data, flags, arr["t"], arr["w"], arr["tinv"], arr["winv"])
    A, TL, SR = _lib.E_ARG, _lib.E_TOO_LARGE, _lib.E_SCALAR_RANGE
    for nm in names:
        assert o(**{nm: None}) == A, nm                                          # a NULL array
        assert o(**{nm: [good[nm][0], None]}) == A, nm                           # a NULL entry
    assert o(null="gamma") == A and o(null="r") == A
    assert o(k=0) == A and o(k=9) == A and o(n_=0) == A
    assert o(field=4) == A and o(field=-1) == A
    assert b"bad field id" in L.nmx_last_error()
    for fl in (_lib.ASYNC, _lib.BASES_MONT, _lib.BASES_DEVICE, _lib.OUT_PARTIAL, 1 << 20, _lib.ASYNC | _lib.SCALARS_DEVICE):
        assert o(flags=fl) == A, fl
    assert o(k=2, n_=1 << 30) == TL and o(k=1, n_=1 << 31) == TL and o(k=8, n_=1 << 28) == TL and o(k=1, n_=1 << 32) == TL and o(k=2, n_=(1 << 63) + 1) == TL
    assert o(gamma=p) == SR and o(r=p) == SR and o(gamma=(1 << 256) - 1) == SR and o(r=p + 1) == SR
    # overlaps: an output over an input (in place, by one element at either end), an output over another output
    assert o(t=[at(0), at(9)]) == A and o(winv=[at(14), at(7, 1)]) == A and o(w=[at(10), at(6, n - 1)]) == A
    assert b"overlap" in L.nmx_last_error()
    assert o(tinv=[at(12), at(8)]) == A and o(tinv=[at(12), at(12, 1)]) == A and o(t=[at(8), at(8, n - 1)]) == A and o(winv=[at(14), at(13, 1)]) == A
    assert b"overlap" in L.nmx_last_error()
    assert (buf == before).all(), "a refused call wrote something"
    # inputs may alias one another; a well-formed call gets past every check: what stops it without a device is NMX_E_NO_DEVICE, nothing else
    with_device = L.nmx_device_count() > 0
    want = (0, _lib.E_ZERO) if with_device else (_lib.E_NO_DEVICE,)
    assert o() in want and o(k=1) in want and o(flags=_lib.SCALARS_MONT) in want and o(L=good["mem"], ts=[at(6), at(6)]) in want
    if not with_device:
        assert (buf == before).all()


# ---- (3) the kernels' lane bodies under the emulation --------------------------------------------------------------------------------
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "ppsnark_oracles_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_ppsnark_oracles_emul.so")
RI = 1 << 261          # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)
R256 = oc.R256         # the Montgomery form of NMX_SCALARS_MONT


@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in ("fp.hpp", "ppsnark_oracles.hpp", "spmv_row.hpp",
                                                                                                            "msm_partition.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.emul_gather.argtypes = [i, vp, u32, vp, u32, u32, vp, vp]
    lib.emul_pps_level0.argtypes = [i, vp, u32, u32, u32, vp, vp, i]
    return lib


def words(vals):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals) or bytes(32), np.uint32).copy()


SLACK = 0xdeadbeef


def emul_gather(E, fid, mem, addr, mont):
    """-> (out as integers, the error word); addr are the stored words (already in the vectors' form)"""
    mw, aw = words(mem), words(addr)
    out = np.full(8 * len(addr) + 8, SLACK, np.uint32)
    err = np.zeros(1, np.uint32)
    assert E.emul_gather(fid, mw.ctypes.data, len(mem), aw.ctypes.data, len(addr), 1 if mont else 0, out.ctypes.data, err.ctypes.data) == 0
    assert (out[8 * len(addr):] == SLACK).all(), "a store past the end of out"
    return out[:8 * len(addr)], int(err[0])


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("mont", [False, True])
def test_emulated_gather(E, fid, mont):
    import random
    p = fc.FIELDS[fid]
    rng = random.Random(11 * fid + mont)
    for n_mem, n in ((1, 1), (1, 300), (300, 1), (257, 1000)):
        mem = [rng.choice([0, p - 1, (1 << 256) - 1]) if rng.random() < 0.1 else rng.randrange(p) for _ in range(n_mem)]   # copied as they are
        addr = [rng.randrange(n_mem) for _ in range(n)]
        addr[0], addr[-1] = n_mem - 1, 0
        out, err = emul_gather(E, fid, mem, oc.to_form(p, addr, mont), mont)
        assert err == 0 and fc.ints(out.view(np.uint8)) == oc.gather(mem, addr), (n_mem, n)
        # a refused address raises the word; every OTHER element is still gathered, the refused one is not written
        for bad in (n_mem, n_mem + 1, (1 << 32) + 1, 1 << 64, p - 1):
            j = rng.randrange(n)
            a2 = oc.to_form(p, addr, mont)
            a2[j] = bad * (R256 if mont else 1) % p
            out, err = emul_gather(E, fid, mem, a2, mont)
            got = fc.ints(out.view(np.uint8))
            assert err == 1 and got[j] == int.from_bytes(np.full(8, SLACK, np.uint32).tobytes(), "little"), (n_mem, n, bad)
            assert got[:j] + got[j + 1:] == oc.gather(mem, addr[:j] + addr[j + 1:])
    # words that are no field elements: at or above p, and all ones (canonical: non-zero high words; Montgomery: refused by the range check
    # even where the word reduces to a valid address: p + 2^256 mod p reduces to the address 1)
    mem = [rng.randrange(p) for _ in range(5)]
    for w in (p, p + 1, (1 << 256) - 1, p + (R256 % p if mont else 1)):
        if w < (1 << 256):
            out, err = emul_gather(E, fid, mem, [w], mont)
            assert err == 1, hex(w)


def emul_oracles(E, fid, case, mont, K):
    """both level-0 passes over case's operands in the form `mont`, the chunk products inverted here in between (which is what the levels
    above deliver: F^2 / P for a stored product P).  -> per memory the four outputs as integers (stored words)"""
    p, k, n = case.p, case.k, case.n
    form = R256 if mont else 1
    Tn = -(-n // K)
    ins = [[words(oc.to_form(p, v, mont)) for v in grp] for grp in (case.mems, case.addrs, case.Ls, case.tss)]
    outs = [[np.full(8 * n + 8, SLACK, np.uint32) for _ in range(k)] for _ in range(4)]          # t, w, tinv, winv
    tab = np.zeros(8 * k, np.uint64)
    for m in range(k):
        tab[8 * m:8 * m + 8] = [ins[0][m].ctypes.data, ins[3][m].ctypes.data, outs[0][m].ctypes.data, outs[2][m].ctypes.data,
                                ins[2][m].ctypes.data, ins[1][m].ctypes.data, outs[1][m].ctypes.data, outs[3][m].ctypes.data]
    consts = words([case.gamma * RI % p, case.r * form % p, form * RI % p, Tn * form % p, RI * RI * pow(form, -1, p) % p])
    chunk = np.full(8 * 2 * k * Tn + 8, SLACK, np.uint32)
    assert E.emul_pps_level0(fid, tab.ctypes.data, k, n, K, consts.ctypes.data, chunk.ctypes.data, 0) == 0
    assert (chunk[8 * 2 * k * Tn:] == SLACK).all(), "a store past the end of the chunk products"
    prods = fc.ints(chunk[:8 * 2 * k * Tn].view(np.uint8))
    # the chunk products are what the definition says: the product of the chunk's stored x words, each further one divided by R
    want = case.want()
    for s in range(2 * k):
        xs = oc.to_form(p, want[s // 2][s % 2], mont)
        for cl in range(Tn):
            el = [xs[i] for i in range(cl, n, Tn)][:K]
            assert len(el) >= 1
            prod = RI
            for x in el:
                prod = prod * x * pow(RI, -1, p) % p
            assert prods[s * Tn + cl] == prod, (s, cl)
    chunk[:8 * 2 * k * Tn] = words([form * form * pow(x, -1, p) % p for x in prods])
    assert E.emul_pps_level0(fid, tab.ctypes.data, k, n, K, consts.ctypes.data, chunk.ctypes.data, 1) == 0
    for grp in outs:
        for o in grp:
            assert (o[8 * n:] == SLACK).all(), "a store past the end of an output"
    return [tuple(fc.ints(outs[j][m][:8 * n].view(np.uint8)) for j in range(4)) for m in range(k)]


def check_emulated(E, fid, case, mont, K):
    p = case.p
    got = emul_oracles(E, fid, case, mont, K)
    assert all(x < p for mem in got for v in mem for x in v), "an output is not the canonical representative"
    assert got == [tuple(oc.to_form(p, v, mont) for v in mem) for mem in case.want()], (fid, mont, case.k, case.n, K)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("mont", [False, True])
def test_emulated_level0_passes(E, fid, mont):
    """n = 1, 7, 8, 9 and 1000 with k = 1 and 2 at the chunk length of these sizes (8): chunks of a single element, a segment of exactly one
    chunk per lane, chunk tails (9 = 2 chunks per segment of 5 and 4 elements; 1000 = 125 chunks of 8), several blocks (k = 2, n = 1000: 500
    lanes), and the T | W and memory boundaries, which fall between lanes"""
    for n in (1, 7, 8, 9, 1000):
        for k in (1, 2):
            check_emulated(E, fid, oc.random_case(fid, k, n, seed=fid + 1), mont, 8)


def test_emulated_level0_other_chunk_lengths_and_edge_contents(E):
    """the chunk lengths of longer vectors (16, 32) on short ones, and the edge contents (mem 0 and p - 1, gamma 0 and p - 1, r = 0, ts 0 and n)"""
    for fid in (1, 2):
        for n, K in ((9, 16), (40, 16), (33, 32), (100, 32), (1000, 32)):
            check_emulated(E, fid, oc.random_case(fid, 2, n, seed=5), False, K)
            check_emulated(E, fid, oc.random_case(fid, 3, n, seed=6), True, K)
        for n in (1, 2, 9, 130):
            for case in oc.edge_cases(fid, 2, n, seed=n):
                check_emulated(E, fid, case, False, 8)
                check_emulated(E, fid, case, True, 8)


def test_emulated_level0_bounds_at_their_worst(E):
    """every entry p - 1 with gamma = p - 1 and r = p - n - 5: T + r = i - n - 4 and W + r = -5, none zero"""
    for fid in sorted(fc.FIELDS):
        p, n = fc.FIELDS[fid], 20
        mems, addrs = [[p - 1] * n], [[n - 1] * n]
        case = oc.Case(fid, 1, n, mems, addrs, [[p - 1] * n], p - 1, p - n - 5)
        check_emulated(E, fid, case, False, 8)
        check_emulated(E, fid, case, True, 8)
