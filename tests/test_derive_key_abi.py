"""nmx_bases_derive_by_address without a GPU.  (1) The entry point is declared with the issue's parameter list behind the fixed-base keys and
before nmx_msm, exported, bound in Python / C++ / Rust (the C++ wrappers also compiled and run, tests/cpp/derive_key_mirror_test.cpp), and the
header names the reference's line ranges, every error code, the flags and derive_lmax.  (2) Every refusal that needs no device returns its code
with no device present and leaves *handle untouched.  (3) The whole chain of nova_amd/csrc/derive_key.hpp (derive_pipeline: DeriveKeysFn, pair
sort, BoundsFn, PlanFn, ExpandFn, AccumFn, the strided FoldFn passes, k_derive_affine) runs under tests/host_emul with limb bounds asserted,
bit-exact against pyref on all four curves: table sizes around the block of 256, one index holding 1, lmax, lmax + 1 and 64 lmax + 1 entries
at derive_lmax = 2, P with -P, the same point twice, an identity source row, an out-of-range device-form address, n = 0 and an all-empty
block.  What the emulation does NOT run: the launches, the rocPRIM sort, the quad forms of accumulate and fold, build_key, the key's window
tables; tests/test_gpu_derive_key.py covers those."""
import ctypes
import inspect
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import derive_key_common as dk
from tests import fixed_base_common as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
PARAMS = ["uint64_t ck_handle", "const uint64_t* addresses", "size_t n", "size_t table_size", "uint32_t flags", "uint64_t* handle"]
CURVE_IDS = [c.name for c in dk.CURVES]


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
    ctype_of = {"uint64_t ck_handle": ctypes.c_uint64, "const uint64_t* addresses": ctypes.c_void_p, "size_t n": ctypes.c_size_t,
                "size_t table_size": ctypes.c_size_t, "uint32_t flags": ctypes.c_uint32, "uint64_t* handle": ctypes.POINTER(ctypes.c_uint64)}
    m = re.search(r"int nmx_bases_derive_by_address\(([^;]*)\);", hdr)
    assert m, "the header does not declare nmx_bases_derive_by_address"
    assert [x.strip() for x in re.sub(r"\s+", " ", m.group(1)).split(",")] == PARAMS
    assert hasattr(L, "nmx_bases_derive_by_address")
    assert list(L.nmx_bases_derive_by_address.argtypes) == [ctype_of[d] for d in PARAMS]
    assert hdr.index("int nmx_bases_setup_from_tau(") < hdr.index("int nmx_bases_derive_by_address(") < hdr.index("int nmx_msm(")
    doc = hdr.split("int nmx_bases_derive_by_address(")[0].rsplit("/* ---- key derived by address", 1)[1]
    for needle in ("commitment.rs:177-194", "pedersen.rs:360-381", "hyperkzg.rs:731-749", "pedersen.rs:346-358", "ck_to_group_elements", "NMX_E_ARG",
                   "NMX_E_HANDLE", "NMX_E_TOO_LARGE", "NMX_E_HIP", "InvalidIndex", "InvalidCommitmentKeyLength", "NMX_SCALARS_DEVICE", "NMX_BASES_PRECOMPUTE",
                   "*handle untouched", "table_size >= 2^31", "n >= 2^31", "table_size == 0", "sharded", "wider than the reference", "derive_lmax",
                   "n == 0", "nmx_field_gather"):
        assert needle in doc, needle
    assert '"derive_lmax"' in hdr.split("int nmx_set_option(")[0].rsplit("/*", 1)[1]
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    assert "pub fn nmx_bases_derive_by_address(" in ffi, "ffi.rs: regenerate with scripts/gen_rust_sys.py"


def test_python_and_cpp_wrappers_exist():
    from nova_amd import provider as P
    sig = inspect.signature(P.CommitmentKey.derive_by_address)
    assert list(sig.parameters) == ["self", "addresses", "table_size", "precompute"] and sig.parameters["precompute"].default is True
    sig = inspect.signature(P.CommitmentEngine.ck_derive_by_address)
    assert list(sig.parameters) == ["self", "ck", "addresses", "table_size", "precompute"] and sig.parameters["precompute"].default is True
    hpp = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read()
    key = hpp.split("class CommitmentKey {")[1].split("template <int CURVE> struct DlogGroupExt")[0]
    assert key.index("static CommitmentKey from_scalars(") < key.index("static CommitmentKey setup_from_tau(") < key.index(
        "CommitmentKey derive_by_address(const uint64_t* addresses, size_t n, size_t table_size, bool precompute = true) const")
    res = hpp.split("namespace resident {")[1]
    assert "inline CommitmentKey derive_by_address(const CommitmentKey& ck, const uint64_t* d_addresses, size_t n, size_t table_size" in res
    assert '#include "derive_key.hpp"' in open(os.path.join(CSRC, "runtime.hpp")).read()
    assert "&fixed_base, &derive," in open(os.path.join(CSRC, "curve_impl.hpp")).read()


def test_cpp_wrappers_compile_and_run(L):
    """tests/cpp/derive_key_mirror_test.cpp built with g++ against the product library: the wrappers' types, the refusals decided before a
    device is leased and, where a device is present, a derivation whose expected points are points of the source key"""
    src = os.path.join(ROOT, "tests", "cpp", "derive_key_mirror_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "derive_key_mirror_test.bin")
    deps = [src, os.path.join(ROOT, "include", "nova_mi355x.hpp"), os.path.join(ROOT, "include", "nova_mi355x.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, src, "-L" + os.path.join(ROOT, "nova_amd"), "-lnova_mi355x",
                               "-Wl,-rpath," + os.path.join(ROOT, "nova_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "derive key mirror ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


# ---- (2) refusals -----------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5EEDFACE0BADF00D
NO_KEY = 0x7fffffff12345  # never a registered handle: what the checks below decide, they decide before the key is looked up


def _call(L, addresses=(0, 1, 2, 3), n=4, table_size=4, flags=0, handle="ok", ck=NO_KEY):
    a = None if addresses is None else np.asarray(addresses, dtype=np.uint64)
    h = ctypes.c_uint64(SENTINEL)
    rc = L.nmx_bases_derive_by_address(ck, None if a is None else a.ctypes.data, n, table_size, flags, None if handle is None else ctypes.byref(h))
    assert h.value == SENTINEL, "a refused call wrote *handle"
    return rc


def test_refusals_need_no_device_and_leave_the_handle_untouched(L):
    from nova_amd import _lib
    A = _lib.E_ARG
    assert _call(L, handle=None) == A
    assert _call(L, addresses=None, n=4) == A
    assert _call(L, table_size=0) == A
    assert _call(L, table_size=1 << 31) == A and _call(L, table_size=(1 << 63) + 4) == A
    # (n = 2^31 host addresses are never read: the range of n is checked first)
    assert _call(L, n=1 << 31, table_size=4) == A
    assert _call(L, flags=_lib.SCALARS_MONT) == A
    for fl in (_lib.BASES_MONT, _lib.BASES_DEVICE, _lib.OUT_PARTIAL, _lib.BASES_VALIDATE, _lib.ASYNC, 1 << 20, 1 << 31):
        assert _call(L, flags=fl) == A, fl
    # a host address equal to table_size in the last position of four; one far above 2^32 whose low word is in range
    assert _call(L, addresses=(0, 1, 2, 4)) == A
    assert _call(L, addresses=((1 << 32) + 1, 1, 2, 3)) == A and _call(L, addresses=(0, 1, (1 << 64) - 1, 3)) == A
    # a well-formed call gets past every argument check: the handle is looked up next, and nothing needed a device so far
    assert _call(L) == _lib.E_HANDLE and _call(L, flags=_lib.SCALARS_DEVICE | _lib.BASES_PRECOMPUTE) == _lib.E_HANDLE
    assert _call(L, addresses=None, n=0) == _lib.E_HANDLE
    if L.nmx_device_count() <= 0:
        assert L.nmx_set_option(b"derive_lmax", 4) == _lib.E_NO_DEVICE


# ---- (3) the chain under the emulation ---------------------------------------------------------------------------------------------------
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "derive_key_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_derive_key_emul.so")
SLACK = 0xdeadbeef


@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in (
        "fp.hpp", "curve.hpp", "curves.hpp", "derive_key.hpp", "fixed_base.hpp", "msm_pipeline.hpp", "msm_partition.hpp", "msm_seg.hpp", "msm_kernels.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.emul_derive.argtypes = [i, vp, u32, vp, vp, u32, u32, u32, vp, vp, vp]
    lib.emul_derive_geometry.argtypes = [vp]
    lib.emul_derive_default_lmax.argtypes = [u32, u32]
    lib.emul_derive_default_lmax.restype = u32
    g = np.zeros(4, np.uint32)
    lib.emul_derive_geometry(g.ctypes.data)
    lib.ERR, lib.IDENT, lib.LMIN, lib.LMAX = (int(x) for x in g)
    return lib


STAT_NAMES = ("lmax", "extra_tasks", "split", "max_tasks", "big", "fold_mask", "launches", "block_launches")


def derive(E, c, scalars, addresses, table_size, lmax=0, form=32, clean=None, src_points=None):
    """the emulated chain over key[i] = scalars[i] G (or src_points) -> (points, flag word, stats); form: 32 = the host's narrowed words,
    64 = the caller's words as the kernel reads them from HBM"""
    pts = fb.expect_points(c, scalars) if src_points is None else src_points
    src = dk.internal_rows(c, pts) if len(pts) else np.zeros((1, 16), np.uint32)
    n = len(addresses)
    a64 = np.asarray(addresses, dtype=np.uint64) if form == 64 and n else None
    a32 = np.asarray(addresses, dtype=np.uint32) if form == 32 and n else None
    out = np.full(16 * table_size + 16, SLACK, np.uint32)
    flags = np.full(2, SLACK, np.uint32)
    stats = np.zeros(8, np.uint32)
    if clean is None:
        clean = 0 if R.INF in pts else 1
    rc = E.emul_derive(c.cid, src.ctypes.data, n, None if a64 is None else a64.ctypes.data, None if a32 is None else a32.ctypes.data, table_size, clean,
                       lmax, out.ctypes.data, flags.ctypes.data, stats.ctypes.data)
    assert rc == 0, "the emulation saw a key above table_size, a value not below n or a write past an allocation: %d" % rc
    assert (out[16 * table_size:] == SLACK).all() and flags[1] == SLACK, "a store past the end of the key or of the flag word"
    return dk.points_from_internal(c, out[:16 * table_size]), int(flags[0]), dict(zip(STAT_NAMES, (int(x) for x in stats)))


def test_default_lmax_rule(E):
    """min(4 x mean bucket, n / 2^14) within [32, 1024]"""
    f = E.emul_derive_default_lmax
    assert (E.LMIN, E.LMAX) == (2, 1024)
    assert f(40, 17) == 32 and f(1 << 20, 1 << 16) == 64 and f(1 << 15, 1) == 32 and f(1 << 20, 1) == 64 and f(1 << 26, 4) == 1024
    assert f((1 << 31) - 1, 1) == 1024 and f(1 << 24, 1 << 20) == 64 and f(1 << 22, 1 << 12) == 256


@pytest.mark.parametrize("c", dk.CURVES, ids=CURVE_IDS)
def test_emulated_table_sizes_around_the_block(E, c):
    """table_size 1, 255, 256, 257 with n = 40 random addresses and scalars i + 1; both address forms give the same key"""
    s = list(range(1, 41))
    for T in (1, 255, 256, 257):
        rng = random.Random(T)
        addr = [rng.randrange(T) for _ in range(40)]
        addr[0], addr[39] = 0, T - 1
        want = dk.expect_points(c, s, addr, T)
        got, flags, st = derive(E, c, s, addr, T)
        assert got == want, T
        assert flags == (E.IDENT if R.INF in want else 0) and (T == 1 or R.INF in want)
        assert st["lmax"] == 32 and st["block_launches"] == 1
        assert st["split"] == (1 if T == 1 else 0)      # 40 points on one index against lmax = 32: two tasks
        got64, flags64, _st = derive(E, c, s, addr, T, form=64)
        assert (got64, flags64) == (got, flags), T


@pytest.mark.parametrize("c", dk.CURVES, ids=CURVE_IDS)
def test_emulated_bucket_sizes_at_lmax_2(E, c):
    """one index holding 1, lmax, lmax + 1 and 64 lmax + 1 entries at derive_lmax = 2: no split, no split, two tasks, 65 tasks (a big bucket:
    the T = 64 pass runs)"""
    for Lh, split, tasks, big in ((1, 0, 0, 0), (2, 0, 0, 0), (3, 1, 2, 0), (129, 1, 65, 1)):
        addr, s = dk.heavy_case(Lh)
        got, flags, st = derive(E, c, s, addr, 8, lmax=2)
        assert got == dk.expect_points(c, s, addr, 8), Lh
        assert flags == E.IDENT                             # indices 1, 2, 4, 6 are empty
        assert (st["lmax"], st["split"], st["extra_tasks"], st["big"]) == (2, split, tasks, big), (Lh, st)
        assert bool(st["fold_mask"] & 4) == bool(big) and st["fold_mask"] & 1, (Lh, st)
        if big:
            assert st["max_tasks"] == 65


@pytest.mark.parametrize("c", dk.CURVES, ids=CURVE_IDS)
def test_emulated_group_law_edges_on_one_index(E, c):
    G = (c.gx, c.gy)
    s = [7, c.r - 7, 5, 5, 9, 9, c.r - 9, 11]
    addr = [0, 0, 1, 1, 2, 2, 2, 3]
    got, flags, _st = derive(E, c, s, addr, 4)
    assert got == [R.INF, R.mul(c, 10, G), R.mul(c, 9, G), R.mul(c, 11, G)] and flags == E.IDENT
    got, flags, _st = derive(E, c, [5, 5], [0, 0], 1)       # the same point twice and nothing else: no identity anywhere
    assert got == [R.mul(c, 10, G)] and flags == 0
    got, flags, _st = derive(E, c, [7, c.r - 7], [0, 0], 1)
    assert got == [R.INF] and flags == E.IDENT


@pytest.mark.parametrize("c", dk.CURVES, ids=CURVE_IDS)
def test_emulated_identity_source_rows_contribute_nothing(E, c):
    s = [3, 0, 4, 0, 5, 0]
    addr = [0, 0, 1, 2, 1, 1]
    got, flags, _st = derive(E, c, s, addr, 3)
    assert R.INF in fb.expect_points(c, s)
    assert got == fb.expect_points(c, [3, 9, 0]) and flags == E.IDENT


@pytest.mark.parametrize("c", dk.CURVES, ids=CURVE_IDS)
def test_emulated_out_of_range_device_address_raises_the_flag_and_reads_nothing_out_of_bounds(E, c):
    """HBM-form addresses equal to table_size, 2^32 + 1 (its low word is in range) and 2^64 - 1: the flag is raised, every sorted key stays at
    most table_size (checked by the emulation's backend) and every other index is what it would have been without those entries"""
    T = 5
    for bad in (T, (1 << 32) + 1, (1 << 64) - 1):
        for pos in (0, 9):
            s = list(range(1, 11))
            addr = [i % T for i in range(10)]
            addr[pos] = bad
            got, flags, _st = derive(E, c, s, addr, T, form=64)
            assert flags & E.ERR, (hex(bad), pos)
            keep = [i for i in range(10) if i != pos]
            assert got == dk.expect_points(c, [s[i] for i in keep], [addr[i] for i in keep], T), (hex(bad), pos)


@pytest.mark.parametrize("c", dk.CURVES, ids=CURVE_IDS)
def test_emulated_no_points_and_all_empty_blocks(E, c):
    """n = 0: table_size identities with nothing launched; table_size = 513 with every address below 256: block 1 is all identity, block 2
    holds one (identity) lane"""
    for T in (1, 257):
        got, flags, st = derive(E, c, [], [], T)
        assert got == [R.INF] * T and flags == E.IDENT and st["launches"] == 0
    rng = random.Random(513)
    s = list(range(1, 41))
    addr = [rng.randrange(256) for _ in range(40)]
    want = dk.expect_points(c, s, addr, 513)
    got, flags, st = derive(E, c, s, addr, 513)
    assert got == want and got[256:] == [R.INF] * 257 and flags == E.IDENT and st["block_launches"] == 1
    # and an index in the last block only
    got, flags, _st = derive(E, c, [6], [512], 513)
    assert got == [R.INF] * 512 + [R.mul(c, 6, (c.gx, c.gy))] and flags == E.IDENT
