"""CPU: nova_amd/csrc/field_dispatch.hpp -- the one place a field id becomes a template argument -- compiled with g++: with_field
calls its lambda once with F() == field for the four fields and hands back what it returns, throws Fail{NMX_E_ARG, "bad field id"}
without calling it for anything else, with_index keeps its own range and message; and spmv_index_mask (spmv_row.hpp) at the
extents either side of the 28-bit boundary."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_field_dispatch_and_index_mask():
    exe = os.path.join(ROOT, "tests", "cpp", "field_dispatch_test.bin")
    src = os.path.join(ROOT, "tests", "cpp", "field_dispatch_test.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src])
    rows = []
    for line in subprocess.check_output([exe], text=True).splitlines():
        head, sep, msg = line.partition(" msg=")  # the message is the rest of the line, blanks included
        rows.append(dict(tok.split("=") for tok in head.split()))
        if sep:
            rows[-1]["msg"] = msg
    e_arg = next(r["e_arg"] for r in rows if "e_arg" in r)
    assert e_arg == "-1"
    ok = [r for r in rows if "field" in r]
    assert [(r["field"], r["seen"], r["ret"], r["calls"], r["side"]) for r in ok] == \
        [(str(f), str(f), str(1000 * f + 7), "1", str(1000 * f + 1)) for f in range(4)]
    bad = [r for r in rows if "bad" in r]
    assert [r["bad"] for r in bad] == ["-1", "4", str(2**31 - 1)]
    for r in bad:
        assert (r["threw"], r["calls"], r["code"], r["msg"]) == ("1", "0", e_arg, "bad field id"), r
    modes = {r["mode"]: r for r in rows if "mode" in r}
    assert [modes[str(m)].get("ret") for m in (1, 2, 3)] == ["1000", "2000", "3000"]
    for m in ("0", "4"):
        assert (modes[m]["threw"], modes[m]["code"], modes[m]["msg"]) == ("1", e_arg, "bad sum-check mode")
    masks = {int(r["extent"]): int(r["mask"]) for r in rows if "extent" in r}
    assert masks == {1: 2**28 - 1, 2**28: 2**28 - 1, 2**28 + 1: 0xffffffff}
