"""nmx_ipa_verify without a GPU.  (1) The yardstick first: tests/ipa_verify_common.restate agrees with tests/ipa_common.verify on
honest proofs of the oracle's prover and rejects every single tamper; the closed form of b_hat equals the eq-table form; the tile
decomposition equals the recurrence of ipa_pc.rs:335-349.  (2) The entry point is exported, bound in Python / C++ / Rust, checks its
arguments before a device is needed and refuses to compute without one.  (3) The kernel's tile body (nova_amd/csrc/ipa_verify.hpp)
runs under tests/host_emul/simt.hpp and must write s byte for byte.  InnerProductArgument::verify: src/provider/ipa_pc.rs:286-390."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import fv_common as C
from tests import ipa_common as ic
from tests import ipa_verify_common as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ipa_verify_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "ipa_verify_mirror_test.bin")
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "ipa_verify_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_ipa_verify_emul.so")
CSRC = os.path.join(ROOT, "nova_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    from nova_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- (1) the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [R.GRUMPKIN, R.PALLAS, R.BN254_G1], ids=lambda c: c.name)
@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_restatement_agrees_with_the_existing_verifier_and_rejects_tampers(curve, n):
    I = V.instance_of(curve, n, seed=40 + n)
    assert ic.verify(curve, I["ck"], np.frombuffer(I["ckc"], np.uint8), I["a"], I["b"], n, I["Ls"], I["Rs"], I["infs"], I["a_hat"], I["rs"])
    res = V.restate_instance(I)
    assert res.verdict is True and len(res.s) == n
    for name, over in V.tampers(I).items():
        bad = V.restate_instance(I, **over)
        assert bad is not None and bad.verdict is False, name
    # a proof for this key checked over a different key
    other = V.instance_of(curve, n, seed=40 + n)
    from oracle import cref
    assert V.restate_instance(I, ck=cref.sequential_bases(curve, 5000, n)).verdict is False
    assert other["Ls"] == I["Ls"]  # (deterministic instances: the GPU tests rebuild them)


def test_restatement_accepts_an_all_zero_witness_with_identity_rounds():
    I = V.instance_of(R.GRUMPKIN, 8, seed=3, zero_a=True)
    assert any(i[0] or i[1] for i in I["infs"]) and I["comm_a"] is R.INF
    assert V.restate_instance(I).verdict is True


@pytest.mark.parametrize("fid", sorted(C.FIELDS))
def test_closed_form_of_b_hat_equals_the_table_form(fid):
    p = C.FIELDS[fid]
    rng = random.Random(900 + fid)
    for ell in range(0, 11):
        rs = [rng.randrange(1, p) for _ in range(ell)]
        point = [rng.randrange(p) for _ in range(ell)]
        eq = R.eq_evals(p, point) if ell else [1]
        s = V.s_vector(p, rs)
        assert len(eq) == len(s) == 1 << ell
        assert V.b_hat_closed(p, point, rs) == sum(x * y for x, y in zip(eq, s)) % p


@pytest.mark.parametrize("fid", sorted(C.FIELDS))
def test_tile_decomposition_equals_the_recurrence(fid):
    p = C.FIELDS[fid]
    rng = random.Random(77 + fid)
    for ell in (0, 1, 3, 8, 9, 11):
        rs = [rng.randrange(1, p) for _ in range(ell)]
        assert V.s_tiled(p, rs) == V.s_vector(p, rs)
        want = [1] * (1 << ell)  # the definition: s[i] = prod_k (bit_{ell-1-k}(i) ? r_k : r_k^-1)
        for i in range(1 << ell):
            for k in range(ell):
                want[i] = want[i] * (rs[k] if (i >> (ell - 1 - k)) & 1 else pow(rs[k], p - 2, p)) % p
        assert V.s_vector(p, rs) == want


# ---- (2) the surface -------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_bound_and_the_flag_is_the_same_everywhere(L):
    from nova_amd import _lib
    assert hasattr(L, "nmx_ipa_verify") and len(L.nmx_ipa_verify.argtypes) == 17
    hdr = open(os.path.join(ROOT, "include", "nova_mi355x.h")).read()
    m = re.search(r"NMX_IPA_B_IS_POINT = 1u << (\d+)", hdr)
    assert m and (1 << int(m.group(1))) == _lib.IPA_B_IS_POINT == 1024
    bits = [int(x) for x in re.findall(r"^\s+NMX_[A-Z_0-9]+ = 1u << (\d+)", hdr.split("/* flags */")[1].split("};")[0], flags=re.M)]
    assert len(bits) == len(set(bits)) >= 11 and 10 in bits  # a bit of its own: no two flags share one
    assert "enum { NMX_IPA_REJECT = 1u << 0 };" in hdr and _lib.IPA_REJECT == 1
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    assert "pub fn nmx_ipa_verify(" in ffi
    assert re.search(r"pub const NMX_IPA_B_IS_POINT: u32 = (1 << 10|1024|0x400);", ffi), "ffi.rs: regenerate with scripts/gen_rust_sys.py"


def test_python_and_cpp_wrappers_exist():
    import inspect
    import nova_amd
    sig = list(inspect.signature(nova_amd.ipa_verify).parameters)
    assert sig[:5] == ["ck", "ck_c_xy64", "comm_a", "c", "b"] and sig[-3:] == ["mont", "point", "want_intermediates"]
    src = inspect.getsource(nova_amd.ipa_verify)
    assert "BASES_MONT if ck.mont" in src
    hpp = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read()
    assert "inline bool verify(const CommitmentKey& ck" in hpp and "inline bool ipa_verify(const CommitmentKey& ck" in hpp
    assert "ck.mont() ? NMX_BASES_MONT" in hpp.split("inline bool verify_call(")[1].split("return verdict == 0;")[0]


def call(L, h=1, ckc=True, comm_a=True, comm_a_inf=0, c=True, b=True, n=4, Lp=True, Rp=True, a_hat=True, rs=True, flags=0, verdict=True, outs=None):
    buf = np.zeros((32, 64), np.uint8)
    buf[:, 0] = 1
    p = buf.ctypes.data
    v = ctypes.c_uint32(0xabcd)
    o = outs if outs is not None else (None, None, None)
    rc = L.nmx_ipa_verify(h, p if ckc else None, p if comm_a else None, comm_a_inf, p if c else None, p if b else None, n, p if Lp else None,
                          p if Rp else None, None, p if a_hat else None, p if rs else None, flags, ctypes.byref(v) if verdict else None, *o)
    return rc, v.value


def test_argument_checks_come_before_a_device_or_a_key(L):
    """every NMX_E_ARG case of the header returns on a machine without a GPU and with a handle that does not exist"""
    from nova_amd import _lib
    E = _lib.E_ARG
    assert call(L, verdict=False)[0] == E
    for kw in (dict(ckc=False), dict(comm_a=False), dict(c=False), dict(b=False), dict(a_hat=False), dict(Lp=False), dict(Rp=False), dict(rs=False)):
        assert call(L, **kw) == (E, 0xabcd), kw
    for n in (0, 3, 6, 1 << 31, 1 << 32, (1 << 31) + 1):                      # :297-303
        assert call(L, n=n) == (E, 0xabcd), n
    for fl in (_lib.ASYNC, _lib.SCALARS_SHARDED, _lib.OUT_PARTIAL, _lib.BASES_DEVICE, 1 << 11,
               _lib.SCALARS_DEVICE | _lib.IPA_B_IS_POINT):
        assert call(L, flags=fl) == (E, 0xabcd), fl
    # what is allowed to be null: comm_a when it is the identity, L / R / rs when there is no round -- these get past the checks
    for kw in (dict(comm_a=False, comm_a_inf=1), dict(n=1, Lp=False, Rp=False, rs=False)):
        rc, v = call(L, h=0xdeadbeef, **kw)
        assert rc in (_lib.E_NO_DEVICE, _lib.E_HANDLE) and v == 0xabcd, kw


def test_refuses_without_a_device_and_leaves_the_outputs_alone(L):
    from nova_amd import _lib
    if L.nmx_device_count() > 0:
        rc, v = call(L, h=0xdeadbeef)   # a device is visible: the unknown key is what stops the call
        assert (rc, v) == (_lib.E_HANDLE, 0xabcd)
        return
    out = np.full(97, 0x5a, np.uint8)
    outs = (out.ctypes.data, out.ctypes.data + 64, out.ctypes.data + 65)
    for fl in (0, _lib.SCALARS_MONT | _lib.BASES_MONT, _lib.IPA_B_IS_POINT):
        rc, v = call(L, flags=fl, outs=outs)
        assert rc == _lib.E_NO_DEVICE and b"no HIP device" in L.nmx_last_error()
        assert v == 0xabcd and (out == 0x5a).all()


def build_cpp():
    import __graft_entry__
    __graft_entry__.build()
    deps = [SRC, os.path.join(ROOT, "include", "nova_mi355x.hpp"), os.path.join(ROOT, "include", "nova_mi355x.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", BIN, SRC,
                               "-L" + os.path.join(ROOT, "nova_amd"), "-lnova_mi355x",
                               "-L" + os.path.join(ROOT, "oracle"), "-lnova_ref",
                               "-Wl,-rpath," + os.path.join(ROOT, "nova_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
                               "-Wl,-rpath,/opt/rocm/lib"])
    return BIN


def test_cpp_mirror_builds_and_refuses_without_gpu(L):
    b = build_cpp()
    if L.nmx_device_count() > 0:
        return  # (a device is visible: the binary runs in tests/test_gpu_ipa_verify.py)
    r = subprocess.run([b], capture_output=True, text=True)
    assert r.returncode == 3, (r.returncode, r.stderr)
    assert "no HIP device" in r.stderr


# ---- (3) the tile body under the emulation --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in ("fp.hpp", "ipa_verify.hpp", "msm_partition.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp = ctypes.c_void_p
    lib.emul_ipa_s.argtypes = [ctypes.c_int, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, vp, vp, vp]
    return lib


def emul_s(E, fid, rs, lo, cnt, grid=0, b=None):
    p = C.FIELDS[fid]
    t0, hs0, rsq = V.kernel_constants(p, rs)
    rq = np.frombuffer(b"".join(ic.le(x) for x in rsq) + bytes(32), np.uint8).copy()
    out = np.full(32 * cnt + 64, 0xee, np.uint8)          # 64 guard bytes: nothing may be written past the range
    lanes = np.zeros(128 * 256 * 32, np.uint8)
    bb = V.b_array(b) if b is not None else None
    g = E.emul_ipa_s(fid, ic.le(t0), ic.le(hs0), rq.ctypes.data, len(rs), lo, cnt, grid, bb.ctypes.data if b is not None else None,
                     out.ctypes.data, lanes.ctypes.data)
    assert g >= 1 and (out[32 * cnt:] == 0xee).all()
    raw = sum(ic.ints(lanes[:g * 256 * 32])) % p
    return ic.ints(out[:32 * cnt]), raw * (1 << 261) % p, g


@pytest.mark.parametrize("fid", sorted(C.FIELDS))
@pytest.mark.parametrize("ell", [0, 1, 8, 9, 13])
def test_emulated_tile_body_writes_s(E, fid, ell):
    p = C.FIELDS[fid]
    rng = random.Random(1000 * fid + ell)
    rs = [rng.randrange(1, p) for _ in range(ell)]
    n = 1 << ell
    want = V.s_vector(p, rs)
    b = [rng.randrange(p) for _ in range(n)]
    b[0], b[-1] = p - 1, p - 1
    got, dot, g = emul_s(E, fid, rs, 0, n, b=b)
    assert got == want
    assert dot == sum(x * y for x, y in zip(b, want)) % p
    assert g == max(1, n // 4096)
    if ell == 13:  # fewer blocks than groups (a block walks two groups), and no b
        got, dot, g = emul_s(E, fid, rs, 0, n, grid=1)
        assert got == want and dot == 0 and g == 1


@pytest.mark.parametrize("fid", sorted(C.FIELDS))
def test_emulated_range_that_starts_and_ends_inside_a_tile(E, fid):
    p = C.FIELDS[fid]
    rng = random.Random(5 + fid)
    rs = [rng.randrange(1, p) for _ in range(13)]
    want = V.s_vector(p, rs)
    for lo, cnt in ((100, 700), (4095, 2), (4097, 4095), (8191, 1), (300, 1 << 12)):
        b = [rng.randrange(p) for _ in range(cnt)]
        got, dot, _g = emul_s(E, fid, rs, lo, cnt, b=b)
        assert got == want[lo:lo + cnt], (lo, cnt)
        assert dot == sum(x * y for x, y in zip(b, want[lo:lo + cnt])) % p
